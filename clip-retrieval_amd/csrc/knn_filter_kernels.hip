// knn_filter_kernels.hip -- the post filter of one large-k request on the device (knnx_search_filtered; include/knnx.h, "Post filter on
// the device"; clip_back.py:290-331).  The k result rows are already in HBM (gathered / decoded by the reconstruct kernels);
// the four kernels here turn them into one byte per result:
//   filter_normalise_kernel  r_i -> e_i = r_i / |r_i| in place, one wave per row; the sum of squares is ONE fmaf chain over the columns in
//                            ascending order (every lane runs the same chain over the row's LDS copy, so no reduction order exists)
//   filter_links_kernel      sim(i, j) = e_i . e_j for the tiles of the upper triangle on v_mfma_f32_32x32x2_f32 -- on gfx950 bit for bit
//                            the k-ordered fmaf chain from +0 -- and every pair i < j < n with sim > thr appended to the link list, one
//                            returning atomic per wave that has hits
//   filter_bits_kernel       violence (first maximum of the prompt scores is prompt 1) and safety (output 0 > thr) bits from the two
//                            score arrays the resident MLPs left on the device
//   filter_cc_kernel         connected components of the links in ONE workgroup, labels in LDS (knnx_filter_plan.h states the rounds);
//                            every rank that is not the smallest of its component gets the duplicate bit
// None of them has scratch (private memory); figures in DESIGN 4.9.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/knnx.h"
#include "knn_kernels.h"
#include "knnx_filter_plan.h"

namespace knnx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- rows -> unit rows ------------------------------------------------------------------------------------------------------------
// block = 4 waves = 4 rows; dynamic LDS: 4 x d floats.  Columns d_user .. d - 1 (the padding of the Python layer; on a compressed index
// whatever the decoder left there) take no part and are written as 0, so that the link kernel may run over whole 32-column chunks.
__global__ __launch_bounds__(256) void filter_normalise_kernel(float* __restrict__ R, int n, int d, int d_user) {
  extern __shared__ float sm_rows[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  const bool live = row < n;  // (wave-uniform)
  float* x = sm_rows + (size_t)w * d;
  float* g = R + (size_t)(live ? row : 0) * d;
  if (live)
    for (int c = lane * 4; c < d; c += 256) *reinterpret_cast<float4*>(x + c) = *reinterpret_cast<const float4*>(g + c);
  __syncthreads();
  if (!live) return;
  float s = 0.f;
  int c = 0;
  for (; c + 4 <= d_user; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + c);
    s = __builtin_fmaf(v.x, v.x, s);
    s = __builtin_fmaf(v.y, v.y, s);
    s = __builtin_fmaf(v.z, v.z, s);
    s = __builtin_fmaf(v.w, v.w, s);
  }
  for (; c < d_user; ++c) s = __builtin_fmaf(x[c], x[c], s);
  const float nrm = s == 0.f ? 1.f : sqrtf(s);  // a zero row stays zero (normalized(), clip_back.py:194-197)
  for (int c2 = lane; c2 < d; c2 += 64) g[c2] = c2 < d_user ? x[c2] / nrm : 0.f;
}

// ---- links ------------------------------------------------------------------------------------------------------------------------
// One workgroup per tile (ti <= tj) of the upper triangle: 64 rows i x 64 rows j, four waves of 32 x 32 each, the two row blocks staged
// through LDS 32 columns at a time.  A operand of lane l: e_i[k] with i = l & 31, k = l >> 5; B operand: e_j[k] with j = l & 31.
constexpr int FL_KC = 32;       // columns per stage
constexpr int FL_LD = FL_KC + 1;  // LDS row stride in floats (odd: the 32 rows a half-wave reads fall into 32 different banks)

__global__ __launch_bounds__(256) void filter_links_kernel(const float* __restrict__ E, int n, int d, int dk, float thr,
                                                          uint32_t* __restrict__ links, int cap, int* __restrict__ counters) {
  __shared__ float sA[FILTER_TILE * FL_LD];
  __shared__ float sB[FILTER_TILE * FL_LD];
  const FilterTileXY t = filter_tile((int)blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
  const int i0 = t.ti * FILTER_TILE, j0 = t.tj * FILTER_TILE;
  // staging: thread -> (row tid / 8 and 32 + tid / 8, columns 4 (tid % 8) .. + 3); rows at or beyond n are read from row n - 1 and zeroed
  const int sr = tid >> 3, sc = (tid & 7) * 4;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < dk; k0 += FL_KC) {
    float4 va[2], vb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ra = i0 + sr + 32 * h, rb = j0 + sr + 32 * h;
      va[h] = *reinterpret_cast<const float4*>(E + (size_t)(ra < n ? ra : n - 1) * d + k0 + sc);
      vb[h] = *reinterpret_cast<const float4*>(E + (size_t)(rb < n ? rb : n - 1) * d + k0 + sc);
      if (ra >= n) va[h] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rb >= n) vb[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // the previous stage has been read
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float* pa = sA + (sr + 32 * h) * FL_LD + sc;
      float* pb = sB + (sr + 32 * h) * FL_LD + sc;
      pa[0] = va[h].x, pa[1] = va[h].y, pa[2] = va[h].z, pa[3] = va[h].w;
      pb[0] = vb[h].x, pb[1] = vb[h].y, pb[2] = vb[h].z, pb[3] = vb[h].w;
    }
    __syncthreads();
    const float* qa = sA + (wm * 32 + (lane & 31)) * FL_LD + (lane >> 5);
    const float* qb = sB + (wn * 32 + (lane & 31)) * FL_LD + (lane >> 5);
#pragma unroll
    for (int kk = 0; kk < FL_KC; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[kk], qb[kk], acc, 0, 0, 0);
  }
  // epilogue: register r of lane l is sim(i, j) with i = (r & 3) + 8 (r >> 2) + 4 (l >> 5), j = l & 31 inside the wave's quadrant
  const int gj = j0 + wn * 32 + (lane & 31);
  const int gi_base = i0 + wm * 32 + 4 * (lane >> 5);
  unsigned hits = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gi = gi_base + (r & 3) + 8 * (r >> 2);
    if (gi < gj && gj < n && acc[r] > thr) hits |= 1u << r;  // the diagonal tile keeps i < j only; j < n implies i < n
  }
  const int mine = __builtin_popcount(hits);
  int incl = mine;  // inclusive scan over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  const int total = __shfl(incl, 63);
  if (total == 0) return;  // wave-uniform
  int base = 0;
  if (lane == 0) base = atomicAdd(counters + FILTER_C_LINKS, total);  // counts every link, also those past the cap
  base = __shfl(base, 0);
  int at = base + incl - mine;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (!(hits >> r & 1u)) continue;
    if (at < cap) links[at] = filter_link(gi_base + (r & 3) + 8 * (r >> 2), gj);
    ++at;
  }
}

// ---- the two score arrays -> bits -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void filter_bits_kernel(const float* __restrict__ vs, int P, const float* __restrict__ ss, int S,
                                                         float sthr, int n, int k, uint8_t* __restrict__ drop) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k) return;
  unsigned bits = 0;
  if (i < n) {
    if (vs) {
      int best = 0;
      float bv = vs[(size_t)i * P];
      for (int p = 1; p < P; ++p) {
        const float v = vs[(size_t)i * P + p];
        if (v > bv) bv = v, best = p;  // strict: the FIRST maximum wins (np.argmax)
      }
      if (best == 1) bits |= KNNX_DROP_VIOLENT;
    }
    if (ss && ss[(size_t)i * S] > sthr) bits |= KNNX_DROP_UNSAFE;
  }
  drop[i] = (uint8_t)bits;
}

// ---- connected components ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void filter_cc_kernel(const uint32_t* __restrict__ links, int cap, int* __restrict__ counters, int n,
                                                        uint8_t* __restrict__ drop) {
  __shared__ int label[FILTER_MAX_K];
  __shared__ int changed;
  const int tid = threadIdx.x;
  const int m = counters[FILTER_C_LINKS];
  if (m <= 0 || m > cap) return;  // nothing to group / more links than were kept: no duplicate bit at all (workgroup-uniform)
  for (int x = tid; x < n; x += 1024) label[x] = x;
  int rounds = 0;
  bool quiet = false;
  while (rounds < n) {  // the hard bound of knnx_filter_plan.h
    if (tid == 0) changed = 0;
    __syncthreads();
    ++rounds;
    for (int e = tid; e < m; e += 1024) {
      const uint32_t l = links[e];
      const int i = filter_link_i(l), j = filter_link_j(l);
      if (i >= n || j >= n) continue;  // (the link kernel writes none such; the labels are 32 KiB of LDS either way)
      const int a = label[i], b = label[j];
      if (a != b) {
        atomicMin(&label[a > b ? a : b], a > b ? b : a);
        changed = 1;
      }
    }
    __syncthreads();
    if (!changed) {
      quiet = true;
      break;
    }
    for (int x = tid; x < n; x += 1024) {
      int r = label[x];
      while (label[r] != r) r = label[r];
      label[x] = r;
    }
    __syncthreads();
  }
  if (tid == 0) {
    counters[FILTER_C_ROUNDS] = rounds;
    counters[FILTER_C_BOUND] = quiet ? 0 : 1;
  }
  if (!quiet) return;
  for (int x = tid; x < n; x += 1024)
    if (label[x] != x) drop[x] |= KNNX_DROP_DUPLICATE;
}

}  // namespace

hipError_t launch_filter_normalise(float* R, int n, int d, int d_user, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (d <= 0 || d % 4 || d_user < 0 || d_user > d || (size_t)d * 16 > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_normalise_kernel, dim3((n + 3) / 4), dim3(256), (size_t)d * 16, st, R, n, d, d_user);
  return hipGetLastError();
}

hipError_t launch_filter_links(const float* E, int n, int d, int d_user, float thr, uint32_t* links, int cap, int* counters, hipStream_t st) {
  if (n <= 1) return hipSuccess;
  const int dk = (d_user + FL_KC - 1) / FL_KC * FL_KC;  // whole stages; the normalise kernel zeroed the columns past d_user
  if (n > FILTER_MAX_K || d % 4 || dk > d || cap < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_links_kernel, dim3(filter_tiles(filter_tiles_side(n))), dim3(256), 0, st, E, n, d, dk, thr, links, cap, counters);
  return hipGetLastError();
}

hipError_t launch_filter_bits(const float* vs, int P, const float* ss, int S, float sthr, int n, int k, uint8_t* drop, hipStream_t st) {
  if (k <= 0) return hipSuccess;
  if (n < 0 || n > k || (vs && P < 1) || (ss && S < 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_bits_kernel, dim3((k + 255) / 256), dim3(256), 0, st, vs, P, ss, S, sthr, n, k, drop);
  return hipGetLastError();
}

hipError_t launch_filter_cc(const uint32_t* links, int cap, int* counters, int n, uint8_t* drop, hipStream_t st) {
  if (n <= 1) return hipSuccess;
  if (n > FILTER_MAX_K || cap < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_cc_kernel, dim3(1), dim3(1024), 0, st, links, cap, counters, n, drop);
  return hipGetLastError();
}

}  // namespace knnx
