// knn_shrink_kernels.hip -- the device half of removing ids from a built IVF index (include/knnx.h, "Shrinking a built index"; DESIGN 4.4;
// the arithmetic is knnx_shrink_plan.h, the host knnx_shrink.hip).  Survivors are renumbered densely in id order and every list is laid
// down again without its dead rows, so rows shift by varying amounts inside a list: the move is ROW-granular, unlike the tile-granular
// move of a growing index (knn_grow_kernels.hip).  The phases are separate launches on one stream; no kernel waits on another workgroup,
// none uses atomics, LDS or scratch:
//   mark      dead[id - id_lo] = 1 for every id of the call that names a row (plain byte stores of one value: duplicates are harmless)
//   rank      block sums of !dead over blocks of SHRINK_BLOCK ids (one wave per block, 16 flag bytes per lane), scanned on the host;
//             then rank[i] = block offset + the exclusive wave scan: the new id of every survivor
//   mask      tmask[t]: the 32-bit survivor mask of source tile t, by a ballot over idmap and dead
//   list scan one wave per list over its tiles' popcounts (4 bytes per tile): tpos[t] = survivors of the list in front of tile t, and
//             the new list sizes, which go to the host for the layout; then tpos[t] += 32 * tile0_new[l] gives dst0[t]
//   move      the survivors of a source tile are one contiguous run of the destination starting at row dst0[t]; the unit of work is a
//             SOURCE tile, never a list -- one 100 k-row list must not serialise the copy.  Every lane owns 16-byte pieces of the source
//             tile; a piece of a dead row is skipped, a piece of a survivor goes to row dst0[t] + shrink_pos(mask, row): loads are
//             contiguous with holes, stores contiguous per run.  Loads are issued ahead of stores, SHRINK_BURST of them per lane.
//             Two shapes, as in the grow move: tiles of at least SHRINK_STEP uint4 get a workgroup per tile (mask and dst0 are
//             wave-uniform, the next tile's are fetched while this one is copied; a fully dead tile costs that one lookup); smaller
//             tiles are walked SHRINK_STEP consecutive source uint4 per step, each lane looking its tile up (neighbours share the entry)
//   pads      rows [size_new[l], 32 * ntile_new[l]) of every list are zeroed, nothing else of the arena is touched twice
//   ids       one thread per source row: idmap_new[dest] = id_lo + rank, inv_new[rank] = dest

#include <hip/hip_runtime.h>

#define KNNX_SHRINK_FN __host__ __device__ inline
#include "knn_kernels.h"
#include "knnx_shrink_plan.h"

namespace knnx {

constexpr int SHRINK_WG = 256;
constexpr int SHRINK_BURST = 4;  // 16-byte loads a lane has in flight before it stores them (written out for 4 below)
constexpr int SHRINK_STEP = SHRINK_WG * SHRINK_BURST;
constexpr int SHRINK_WG_PER_CU = 8;
static_assert(SHRINK_BLOCK == 64 * 16, "a block of the rank scan is one wave of 16-byte lanes");

__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_mark_kernel(const int64_t* __restrict__ ids, int64_t m, int64_t id_lo, int64_t n,
                                                                     uint8_t* __restrict__ dead) {
  const int64_t i = (int64_t)blockIdx.x * SHRINK_WG + threadIdx.x;
  if (i >= m) return;
  const uint64_t o = shrink_index(ids[i], id_lo, n);
  if (o < (uint64_t)n) dead[o] = 1;
}

// the survivors among a lane's 16 ids [base, base + 16): the flags are 0 / 1 bytes, and the bytes past n are never set
__device__ __forceinline__ unsigned shrink_alive16(const uint4 v, int64_t base, int64_t n) {
  const int64_t left = n - base;
  const unsigned valid = left >= 16 ? 16u : left > 0 ? (unsigned)left : 0u;
  return valid - (unsigned)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
}

// dead is allocated in whole blocks: one wave per block, blocksum[b] = its survivors
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_rank_sum_kernel(const uint4* __restrict__ dead16, int64_t n, int64_t nblk,
                                                                         uint32_t* __restrict__ blocksum) {
  const int64_t w = ((int64_t)blockIdx.x * SHRINK_WG + threadIdx.x) >> 6;
  const unsigned lane = threadIdx.x & 63;
  if (w >= nblk) return;  // (a whole wave)
  unsigned c = shrink_alive16(dead16[w * 64 + lane], w * SHRINK_BLOCK + lane * 16, n);
  for (int s = 32; s; s >>= 1) c += __shfl_xor(c, s, 64);
  if (lane == 0) blocksum[w] = c;
}

// rank [whole blocks]: rank[i] = blockoff[i / SHRINK_BLOCK] + survivors of the block in front of i (entries past n are never read)
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_rank_apply_kernel(const uint4* __restrict__ dead16, int64_t n, int64_t nblk,
                                                                           const uint32_t* __restrict__ blockoff, uint4* __restrict__ rank4) {
  const int64_t w = ((int64_t)blockIdx.x * SHRINK_WG + threadIdx.x) >> 6;
  const unsigned lane = threadIdx.x & 63;
  if (w >= nblk) return;
  const uint4 v = dead16[w * 64 + lane];
  const unsigned mine = shrink_alive16(v, w * SHRINK_BLOCK + lane * 16, n);
  unsigned incl = mine;
  for (int s = 1; s < 64; s <<= 1) {
    const unsigned up = __shfl_up(incl, s, 64);
    if (lane >= (unsigned)s) incl += up;
  }
  unsigned run = blockoff[w] + incl - mine;
  const unsigned word[4] = {v.x, v.y, v.z, v.w};
  uint4* out = rank4 + (w * 64 + lane) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint4 r;
    r.x = run, run += 1u - (word[k] & 1u);
    r.y = run, run += 1u - ((word[k] >> 8) & 1u);
    r.z = run, run += 1u - ((word[k] >> 16) & 1u);
    r.w = run, run += 1u - ((word[k] >> 24) & 1u);
    out[k] = r;
  }
}

// prow is a multiple of 32; a wave covers two tiles
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_mask_kernel(const int64_t* __restrict__ idmap, int64_t prow, int64_t id_lo, int64_t n,
                                                                     const uint8_t* __restrict__ dead, uint32_t* __restrict__ tmask) {
  const int64_t r = (int64_t)blockIdx.x * SHRINK_WG + threadIdx.x;
  bool alive = false;
  if (r < prow) {
    const uint64_t o = shrink_index(idmap[r], id_lo, n);
    alive = o < (uint64_t)n && dead[o] == 0;
  }
  const unsigned long long b = __ballot(alive);
  const unsigned lane = threadIdx.x & 63;
  if (r < prow && (lane & 31) == 0) tmask[r >> 5] = (uint32_t)(lane ? b >> 32 : b);
}

// one wave per list (4 bytes per tile: a long list costs a few dozen wave steps)
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_list_scan_kernel(const unsigned* __restrict__ tile0, const unsigned* __restrict__ ntile,
                                                                          int nlist, const uint32_t* __restrict__ tmask, uint32_t* __restrict__ tpos,
                                                                          unsigned* __restrict__ size_new) {
  const int l = (int)((blockIdx.x * SHRINK_WG + threadIdx.x) >> 6);
  const unsigned lane = threadIdx.x & 63;
  if (l >= nlist) return;
  const unsigned t0 = tile0[l], nt = ntile[l];
  unsigned run = 0;
  for (unsigned o = 0; o < nt; o += 64) {  // (wave-uniform trip count)
    const bool in = o + lane < nt;
    const unsigned c = in ? (unsigned)__popc(tmask[t0 + o + lane]) : 0u;
    unsigned incl = c;
    for (int s = 1; s < 64; s <<= 1) {
      const unsigned up = __shfl_up(incl, s, 64);
      if (lane >= (unsigned)s) incl += up;
    }
    if (in) tpos[t0 + o + lane] = run + incl - c;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) size_new[l] = run;
}

__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_dst0_kernel(const unsigned* __restrict__ tile0_old, const unsigned* __restrict__ ntile_old,
                                                                     const unsigned* __restrict__ tile0_new, int nlist, uint32_t* __restrict__ tpos) {
  const int l = (int)((blockIdx.x * SHRINK_WG + threadIdx.x) >> 6);
  const unsigned lane = threadIdx.x & 63;
  if (l >= nlist) return;
  const unsigned t0 = tile0_old[l], nt = ntile_old[l], add = 32u * tile0_new[l];
  for (unsigned o = lane; o < nt; o += 64) tpos[t0 + o] += add;
}

// piece j of a source tile (q4 uint4 per row, 32 q4 per tile) -> its uint4 in the destination, or SHRINK_NONE for a piece of a dead row
constexpr size_t SHRINK_NONE = ~(size_t)0;
__device__ __forceinline__ size_t shrink_piece(unsigned j, unsigned q4, int sh4, uint32_t mask, uint32_t d0) {
  const unsigned row = sh4 >= 0 ? j >> sh4 : j / q4;
  return (mask >> row) & 1u ? (size_t)(d0 + shrink_pos(mask, row)) * q4 + (j - row * q4) : SHRINK_NONE;
}

// the piece at p when it has a destination (a piece without one is never stored)
__device__ __forceinline__ uint4 shrink_load(const uint4* __restrict__ p, size_t at) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (at != SHRINK_NONE) v = *p;
  return v;
}

// large tiles: a workgroup per source tile
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_move_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                     const uint32_t* __restrict__ tmask, const uint32_t* __restrict__ dst0,
                                                                     unsigned tiles, unsigned q4, int sh4) {
  const unsigned q = 32u * q4;
  unsigned t = blockIdx.x;
  uint32_t m = t < tiles ? tmask[t] : 0u, d0 = t < tiles ? dst0[t] : 0u;
  while (t < tiles) {
    const unsigned t_next = t + gridDim.x;
    const uint32_t m_next = t_next < tiles ? tmask[t_next] : 0u, d_next = t_next < tiles ? dst0[t_next] : 0u;  // (in flight while this tile is copied)
    if (m) {
      const uint4* sp = src + (size_t)t * q;
      for (unsigned j = threadIdx.x; j < q; j += SHRINK_STEP) {  // the loads first, then the stores
        const unsigned j1 = j + SHRINK_WG, j2 = j + 2 * SHRINK_WG, j3 = j + 3 * SHRINK_WG;
        const size_t a0 = shrink_piece(j, q4, sh4, m, d0), a1 = j1 < q ? shrink_piece(j1, q4, sh4, m, d0) : SHRINK_NONE,
                     a2 = j2 < q ? shrink_piece(j2, q4, sh4, m, d0) : SHRINK_NONE, a3 = j3 < q ? shrink_piece(j3, q4, sh4, m, d0) : SHRINK_NONE;
        const uint4 v0 = shrink_load(sp + j, a0), v1 = shrink_load(sp + j1, a1), v2 = shrink_load(sp + j2, a2), v3 = shrink_load(sp + j3, a3);
        if (a0 != SHRINK_NONE) dst[a0] = v0;
        if (a1 != SHRINK_NONE) dst[a1] = v1;
        if (a2 != SHRINK_NONE) dst[a2] = v2;
        if (a3 != SHRINK_NONE) dst[a3] = v3;
      }
    }
    t = t_next, m = m_next, d0 = d_next;
  }
}

// source uint4 i of the arena: its tile's mask and dst0 looked up, then as above
__device__ __forceinline__ size_t shrink_small_piece(size_t i, size_t total, unsigned q, unsigned q4, int sh4, const uint32_t* __restrict__ tmask,
                                                     const uint32_t* __restrict__ dst0) {
  if (i >= total) return SHRINK_NONE;
  const size_t t = sh4 >= 0 ? i >> (sh4 + 5) : i / q;
  return shrink_piece((unsigned)(i - t * q), q4, sh4, tmask[t], dst0[t]);
}

// small tiles (q = 32 q4 uint4 per tile, any q4): SHRINK_STEP consecutive source uint4 per step, several tiles
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_move_small_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                           const uint32_t* __restrict__ tmask, const uint32_t* __restrict__ dst0,
                                                                           size_t total, unsigned q4, int sh4, unsigned nsteps) {
  const unsigned q = 32u * q4;
  for (unsigned step = blockIdx.x; step < nsteps; step += gridDim.x) {
    const size_t i0 = (size_t)step * SHRINK_STEP + threadIdx.x, i1 = i0 + SHRINK_WG, i2 = i0 + 2 * SHRINK_WG, i3 = i0 + 3 * SHRINK_WG;
    const size_t a0 = shrink_small_piece(i0, total, q, q4, sh4, tmask, dst0), a1 = shrink_small_piece(i1, total, q, q4, sh4, tmask, dst0),
                 a2 = shrink_small_piece(i2, total, q, q4, sh4, tmask, dst0), a3 = shrink_small_piece(i3, total, q, q4, sh4, tmask, dst0);
    const uint4 v0 = shrink_load(src + i0, a0), v1 = shrink_load(src + i1, a1), v2 = shrink_load(src + i2, a2), v3 = shrink_load(src + i3, a3);
    if (a0 != SHRINK_NONE) dst[a0] = v0;
    if (a1 != SHRINK_NONE) dst[a1] = v1;
    if (a2 != SHRINK_NONE) dst[a2] = v2;
    if (a3 != SHRINK_NONE) dst[a3] = v3;
  }
}

// a workgroup per list: its pad rows, at most 31
__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_pads_kernel(uint4* __restrict__ dst, const unsigned* __restrict__ tile0,
                                                                     const unsigned* __restrict__ ntile, const unsigned* __restrict__ size, unsigned q4) {
  const unsigned l = blockIdx.x;
  const unsigned rows = 32u * ntile[l] - size[l];
  uint4* p = dst + ((size_t)32 * tile0[l] + size[l]) * q4;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (unsigned j = threadIdx.x; j < rows * q4; j += SHRINK_WG) p[j] = zero;
}

__global__ __launch_bounds__(SHRINK_WG) void ivf_shrink_ids_kernel(const int64_t* __restrict__ idmap_old, int64_t prow_old, int64_t id_lo, int64_t n,
                                                                    const uint32_t* __restrict__ tmask, const uint32_t* __restrict__ dst0,
                                                                    const uint32_t* __restrict__ rank, int64_t* __restrict__ idmap,
                                                                    uint32_t* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * SHRINK_WG + threadIdx.x;
  if (r >= prow_old) return;
  const uint32_t m = tmask[r >> 5];
  const unsigned b = (unsigned)(r & 31);
  if (!((m >> b) & 1u)) return;
  const uint64_t o = shrink_index(idmap_old[r], id_lo, n);  // (in range: the mask bit says so)
  const uint32_t dest = dst0[r >> 5] + shrink_pos(m, b), rk = rank[o];
  idmap[dest] = id_lo + (int64_t)rk;
  inv[rk] = dest;
}

static unsigned grid_of(int64_t threads) { return (unsigned)((threads + SHRINK_WG - 1) / SHRINK_WG); }

hipError_t launch_ivf_shrink_mark(const int64_t* ids, int64_t m, int64_t id_lo, int64_t n, uint8_t* dead, hipStream_t st) {
  if (m <= 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_shrink_mark_kernel, dim3(grid_of(m)), dim3(SHRINK_WG), 0, st, ids, m, id_lo, n, dead);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_rank_sum(const uint8_t* dead, int64_t n, uint32_t* blocksum, hipStream_t st) {
  const int64_t nblk = shrink_blocks(n);
  if (nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_shrink_rank_sum_kernel, dim3(grid_of(nblk * 64)), dim3(SHRINK_WG), 0, st, (const uint4*)dead, n, nblk, blocksum);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_rank_apply(const uint8_t* dead, int64_t n, const uint32_t* blockoff, uint32_t* rank, hipStream_t st) {
  const int64_t nblk = shrink_blocks(n);
  if (nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_shrink_rank_apply_kernel, dim3(grid_of(nblk * 64)), dim3(SHRINK_WG), 0, st, (const uint4*)dead, n, nblk, blockoff,
                     (uint4*)rank);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_mask(const int64_t* idmap, int64_t prow, int64_t id_lo, int64_t n, const uint8_t* dead, uint32_t* tmask,
                                  hipStream_t st) {
  if (prow <= 0) return hipSuccess;
  if (prow % 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_shrink_mask_kernel, dim3(grid_of(prow)), dim3(SHRINK_WG), 0, st, idmap, prow, id_lo, n, dead, tmask);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_list_scan(const unsigned* tile0, const unsigned* ntile, int nlist, const uint32_t* tmask, uint32_t* tpos,
                                       unsigned* size_new, hipStream_t st) {
  if (nlist <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_shrink_list_scan_kernel, dim3(grid_of((int64_t)nlist * 64)), dim3(SHRINK_WG), 0, st, tile0, ntile, nlist, tmask, tpos,
                     size_new);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_dst0(const unsigned* tile0_old, const unsigned* ntile_old, const unsigned* tile0_new, int nlist, uint32_t* tpos,
                                  hipStream_t st) {
  if (nlist <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_shrink_dst0_kernel, dim3(grid_of((int64_t)nlist * 64)), dim3(SHRINK_WG), 0, st, tile0_old, ntile_old, tile0_new, nlist,
                     tpos);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_move(const void* src, void* dst, int width, const uint32_t* tmask, const uint32_t* dst0, int64_t tiles, int n_cu,
                                  hipStream_t st) {
  if (tiles <= 0) return hipSuccess;
  if (width <= 0 || width % 16 != 0 || width > 65536 || tiles > (int64_t)0x7ffffffll) return hipErrorInvalidValue;
  const unsigned q4 = (unsigned)width / 16, q = 32u * q4;
  const int sh4 = (q4 & (q4 - 1)) == 0 ? __builtin_ctz(q4) : -1;
  const unsigned cap = (unsigned)std::max(n_cu, 1) * SHRINK_WG_PER_CU;
  if (q < (unsigned)SHRINK_STEP) {
    const size_t total = (size_t)tiles * q;
    const unsigned nsteps = (unsigned)((total + SHRINK_STEP - 1) / SHRINK_STEP);  // (tiles < 2^27, q < 2^10: below 2^27)
    hipLaunchKernelGGL(ivf_shrink_move_small_kernel, dim3(std::min(nsteps, cap)), dim3(SHRINK_WG), 0, st, (const uint4*)src, (uint4*)dst, tmask,
                       dst0, total, q4, sh4, nsteps);
  } else {
    hipLaunchKernelGGL(ivf_shrink_move_kernel, dim3(std::min((unsigned)tiles, cap)), dim3(SHRINK_WG), 0, st, (const uint4*)src, (uint4*)dst,
                       tmask, dst0, (unsigned)tiles, q4, sh4);
  }
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_pads(void* dst, int width, const unsigned* tile0, const unsigned* ntile, const unsigned* size, int nlist,
                                  hipStream_t st) {
  if (nlist <= 0) return hipSuccess;
  if (width <= 0 || width % 16 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_shrink_pads_kernel, dim3((unsigned)nlist), dim3(SHRINK_WG), 0, st, (uint4*)dst, tile0, ntile, size, (unsigned)width / 16);
  return hipGetLastError();
}

hipError_t launch_ivf_shrink_ids(const int64_t* idmap_old, int64_t prow_old, int64_t id_lo, int64_t n, const uint32_t* tmask,
                                 const uint32_t* dst0, const uint32_t* rank, int64_t* idmap, uint32_t* inv, hipStream_t st) {
  if (prow_old <= 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_shrink_ids_kernel, dim3(grid_of(prow_old)), dim3(SHRINK_WG), 0, st, idmap_old, prow_old, id_lo, n, tmask, dst0, rank,
                     idmap, inv);
  return hipGetLastError();
}

}  // namespace knnx
