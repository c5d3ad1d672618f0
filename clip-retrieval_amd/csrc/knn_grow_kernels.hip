// knn_grow_kernels.hip -- the arena move of a growing IVF index (include/knnx.h, "Growing a built index"; the host plan is
// knnx_grow_plan.h).  When lists gain rows the dense layout shifts, so every payload (fp16 rows, PQ codes, SQ8 codes) is copied tile by
// tile from the old arena into a new one, and idmap / inv are rewritten for the rows that moved.
//
// The unit of work is a DESTINATION tile (32 rows x width bytes, always a multiple of 16 bytes: q = 2 width uint4 per tile, q % 32 == 0),
// never a list: one 100 k-row list must not serialise the copy.  src_tile[t] (4 bytes per tile, made by the host with the layout) names
// the old tile a new tile is copied from, GROW_NO_TILE where it has none and is zeroed -- a list's last, partly filled tile travels with
// its pad rows.  A grid sized to the CUs strides over steps; every lane moves GROW_BURST x 16 bytes per step, the loads issued before
// the stores, and every load and store of a wave is one contiguous 1 KiB run.  Two shapes of a step:
//   * tiles of at least GROW_STEP uint4 (16 KiB: fp16 rows, SQ8 codes of d >= 512): a step is one tile, walked by the workgroup in
//     bursts; the source of the NEXT tile is fetched before the current one is copied, so the dependent lookup is off the critical path.
//   * smaller tiles (q a power of two: PQ codes, SQ8 codes of d = 256): a step is GROW_STEP consecutive uint4 of the destination,
//     GROW_STEP / q whole tiles; a lane finds the tile of each of its uint4 by a shift and looks its source up (neighbouring lanes share
//     the entry).  Without this a 2 KiB tile of M = 64 codes left 7 of 8 waves of a step idle behind one lookup.
// No LDS, no atomics.

#include <hip/hip_runtime.h>

#include "knn_kernels.h"
#include "knnx_grow_plan.h"

namespace knnx {

constexpr int GROW_WG = 256;
constexpr int GROW_BURST = 4;     // 16-byte loads a lane has in flight before it stores them (the loops below are written out for 4)
constexpr int GROW_STEP = GROW_WG * GROW_BURST;  // uint4 of one step
constexpr int GROW_WG_PER_CU = 8;

__global__ __launch_bounds__(GROW_WG) void ivf_grow_move_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                 const uint32_t* __restrict__ src_tile, unsigned tiles, unsigned q) {
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  unsigned t = blockIdx.x;
  uint32_t s = t < tiles ? src_tile[t] : GROW_NO_TILE;
  while (t < tiles) {
    const unsigned t_next = t + gridDim.x;
    const uint32_t s_next = t_next < tiles ? src_tile[t_next] : GROW_NO_TILE;  // (in flight while this tile is copied)
    uint4* dp = dst + (size_t)t * q;
    if (s == GROW_NO_TILE) {
      for (unsigned j = threadIdx.x; j < q; j += GROW_WG) dp[j] = zero;
    } else {
      const uint4* sp = src + (size_t)s * q;
      unsigned j = threadIdx.x;
      for (; j + (GROW_BURST - 1) * GROW_WG < q; j += GROW_STEP) {  // whole bursts: the loads first, then the stores
        const uint4 a = sp[j], b = sp[j + GROW_WG], c = sp[j + 2 * GROW_WG], e = sp[j + 3 * GROW_WG];
        dp[j] = a, dp[j + GROW_WG] = b, dp[j + 2 * GROW_WG] = c, dp[j + 3 * GROW_WG] = e;
      }
      for (; j < q; j += GROW_WG) dp[j] = sp[j];
    }
    t = t_next, s = s_next;
  }
}

// one uint4 of the destination: its tile by a shift (q = 1 << qshift), that tile's source, the uint4 at the same place in it -- or zero
__device__ __forceinline__ uint4 grow_fetch(const uint4* __restrict__ src, const uint32_t* __restrict__ src_tile, size_t i, size_t total,
                                            unsigned qshift) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (i < total) {
    const uint32_t s = src_tile[i >> qshift];
    if (s != GROW_NO_TILE) v = src[((size_t)s << qshift) + (i & (((size_t)1 << qshift) - 1))];
  }
  return v;
}

__global__ __launch_bounds__(GROW_WG) void ivf_grow_move_small_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                       const uint32_t* __restrict__ src_tile, size_t total, unsigned qshift,
                                                                       unsigned nsteps) {
  for (unsigned step = blockIdx.x; step < nsteps; step += gridDim.x) {
    const size_t i = (size_t)step * GROW_STEP + threadIdx.x;
    const uint4 a = grow_fetch(src, src_tile, i, total, qshift), b = grow_fetch(src, src_tile, i + GROW_WG, total, qshift),
                c = grow_fetch(src, src_tile, i + 2 * GROW_WG, total, qshift), e = grow_fetch(src, src_tile, i + 3 * GROW_WG, total, qshift);
    if (i < total) dst[i] = a;
    if (i + GROW_WG < total) dst[i + GROW_WG] = b;
    if (i + 2 * GROW_WG < total) dst[i + 2 * GROW_WG] = c;
    if (i + 3 * GROW_WG < total) dst[i + 3 * GROW_WG] = e;
  }
}

// idmap / inv of the new arena: one thread per padded row.  A row of a moved tile keeps its id (-1 on the pad rows it had), every other row
// gets -1 until the appended rows are scattered over it; inv[id - id_lo] of a moved row = its new arena row.
__global__ __launch_bounds__(GROW_WG) void ivf_grow_ids_kernel(const int64_t* __restrict__ idmap_old, const uint32_t* __restrict__ src_tile,
                                                                int64_t prow, int64_t id_lo, int64_t n_ids, int64_t* __restrict__ idmap,
                                                                uint32_t* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * GROW_WG + threadIdx.x;
  if (r >= prow) return;
  const uint32_t s = src_tile[r >> 5];
  const int64_t id = s == GROW_NO_TILE ? -1 : idmap_old[(size_t)s * 32 + (size_t)(r & 31)];
  idmap[r] = id;
  if (id >= id_lo && id - id_lo < n_ids) inv[id - id_lo] = (uint32_t)r;
}

hipError_t launch_ivf_grow_move(const void* src, void* dst, int width, const uint32_t* src_tile, int64_t tiles, int n_cu, hipStream_t st) {
  if (tiles <= 0) return hipSuccess;
  if (width <= 0 || width % 16 != 0 || tiles > (int64_t)0x7ffffffll) return hipErrorInvalidValue;
  const unsigned q = (unsigned)width * 2;  // uint4 per tile
  const unsigned cap = (unsigned)std::max(n_cu, 1) * GROW_WG_PER_CU;
  if (q < (unsigned)GROW_STEP && (q & (q - 1)) == 0) {
    const size_t total = (size_t)tiles * q;
    const unsigned nsteps = (unsigned)((total + GROW_STEP - 1) / GROW_STEP);  // (tiles < 2^27, q < 2^10: below 2^27)
    hipLaunchKernelGGL(ivf_grow_move_small_kernel, dim3(std::min(nsteps, cap)), dim3(GROW_WG), 0, st, (const uint4*)src, (uint4*)dst, src_tile,
                       total, (unsigned)__builtin_ctz(q), nsteps);
  } else {
    hipLaunchKernelGGL(ivf_grow_move_kernel, dim3(std::min((unsigned)tiles, cap)), dim3(GROW_WG), 0, st, (const uint4*)src, (uint4*)dst, src_tile,
                       (unsigned)tiles, q);
  }
  return hipGetLastError();
}

hipError_t launch_ivf_grow_ids(const int64_t* idmap_old, const uint32_t* src_tile, int64_t prow, int64_t id_lo, int64_t n_ids, int64_t* idmap,
                               uint32_t* inv, hipStream_t st) {
  if (prow <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_grow_ids_kernel, dim3((unsigned)((prow + GROW_WG - 1) / GROW_WG)), dim3(GROW_WG), 0, st, idmap_old, src_tile, prow,
                     id_lo, n_ids, idmap, inv);
  return hipGetLastError();
}

}  // namespace knnx
