// knn_idorder_kernels.hip -- list-ordered ids of an IVF index (include/knnx.h, "List-ordered ids"): the export of the mapping in
// ordinal order and the translation of a request's ids.  Both are one thread per element, wave64, 256 threads per workgroup: consecutive
// lanes take consecutive elements, so the staged side (the slice of new_to_old / old_to_new, a request's ids) is read and written
// coalesced and the work of a workgroup is 256 elements whatever the sizes of the lists they fall into.  What is not coalesced is in
// the nature of the mapping: the export reads idmap contiguously inside a list (a wave crosses a list boundary at most every few rows),
// the translation gathers inv[id] for arbitrary ids.  The list of an element comes from a binary search over tile0 / dense0 (nlist
// entries, 256 / 512 KiB at nlist = 65 536: L2-resident; at most 17 steps) -- knnx_id_order.h has the search, shared with the host.

#include <hip/hip_runtime.h>

#define KNNX_IDO_FN __host__ __device__ inline
#include "knnx_id_order.h"
#include "knn_kernels.h"

namespace knnx {

constexpr int IDO_WG = 256;

// out[t] = the id of ordinal o0 + t, t < n (o0 + n <= ntotal): new_to_old[o0 .. o0 + n)
__global__ __launch_bounds__(IDO_WG) void ivf_new_to_old_kernel(const int64_t* __restrict__ idmap, int64_t prow,
                                                                 const unsigned* __restrict__ tile0, const int64_t* __restrict__ dense0,
                                                                 int nlist, int64_t o0, int64_t n, int64_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * IDO_WG + threadIdx.x;
  if (t >= n) return;
  const int64_t row = ido_row_of_ordinal(tile0, dense0, nlist, o0 + t);
  out[t] = row < prow ? idmap[row] : -1;
}

// out[t] = id_base + the ordinal of the row whose id is ids[t] (ids == null: id_base + i0 + t -- old_to_new[i0 .. i0 + n) of the export);
// -1 passes through.  The host has checked the range; an id outside it still reads nothing and answers -1.  out may be ids.
__global__ __launch_bounds__(IDO_WG) void ivf_map_ids_kernel(const uint32_t* __restrict__ inv, int64_t id_base, int64_t ntotal,
                                                              const unsigned* __restrict__ tile0, const int64_t* __restrict__ dense0,
                                                              int nlist, const int64_t* ids, int64_t i0, int64_t n, int64_t* out) {
  const int64_t t = (int64_t)blockIdx.x * IDO_WG + threadIdx.x;
  if (t >= n) return;
  const int64_t u = ids ? ids[t] - id_base : i0 + t;  // (the host's range check keeps ids[t] - id_base from wrapping)
  int64_t r = -1;
  if (!(ids && ids[t] == -1) && u >= 0 && u < ntotal) r = id_base + ido_ordinal_of_row(tile0, dense0, nlist, inv[u]);
  out[t] = r;
}

hipError_t launch_ivf_new_to_old(const int64_t* idmap, int64_t prow, const unsigned* tile0, const int64_t* dense0, int nlist, int64_t o0,
                                 int64_t n, int64_t* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_new_to_old_kernel, dim3((unsigned)((n + IDO_WG - 1) / IDO_WG)), dim3(IDO_WG), 0, st, idmap, prow, tile0, dense0,
                     nlist, o0, n, out);
  return hipGetLastError();
}

hipError_t launch_ivf_map_ids(const uint32_t* inv, int64_t id_base, int64_t ntotal, const unsigned* tile0, const int64_t* dense0, int nlist,
                              const int64_t* ids_or_null, int64_t i0, int64_t n, int64_t* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ivf_map_ids_kernel, dim3((unsigned)((n + IDO_WG - 1) / IDO_WG)), dim3(IDO_WG), 0, st, inv, id_base, ntotal, tile0,
                     dense0, nlist, ids_or_null, i0, n, out);
  return hipGetLastError();
}

}  // namespace knnx
