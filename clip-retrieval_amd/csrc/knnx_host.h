// knnx_host.h -- shared by the HOST translation units of the search half (knnx_api / knnx_range / knnx_ivf / knnx_ivfpq /
// knnx_ivfsq / knnx_grow / knnx_shrink / knnx_filter / knnx_sharded .hip): the error helpers, the owners of device memory, pinned memory, streams and events (hip_owners.h), the index object
// with its state grouped by the scan that uses it, and the handful of functions one file calls in another.  The kernel
// files include knn_kernels.h only.
//
// Allocation rule: every group has ONE alloc() that leaves the whole group allocated or leaves it EMPTY and returns the
// hipError_t; the caller turns that into its error code or its fallback.  Nothing is freed by hand: a group is emptied by
// assigning a fresh one, the index by `delete`.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/knnx.h"
#include "knn_kernels.h"
#include "hip_owners.h"
#include "knnx_filter_plan.h"

using namespace knnx;  // (the launchers and constants of knn_kernels.h)

#pragma GCC visibility push(hidden)  // nothing below is part of the library's ABI

inline thread_local std::string g_err;  // knnx_last_error()
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      return fail(_e == hipErrorOutOfMemory ? KNNX_E_NOMEM : KNNX_E_HIP,                         \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                             \
  } while (0)

// ---- the index: state grouped by the scan that uses it --------------------------------------------
constexpr int IVFM_BLK = 8;                       // 32-query blocks of one multi-block IVF pass (knnx_ivf.hip)
constexpr int PQ_PASS = IVFM_BLK * KNN_NQ;        // queries of one IVF-PQ pass (knnx_ivfpq.hip)
constexpr int PQ_TARGET_WG = 1024;                // ADC workgroups a pass aims for (a query's lists are split over ceil(1024 / nq))
constexpr int PQ_MAX_SPLIT = 128;                 // ... at most (the merge holds split x k scores of a query in the LDS)
constexpr int PQ_SLOTS = PQ_TARGET_WG + PQ_PASS;  // >= nq * split
constexpr int64_t IVFB_CHUNK = (int64_t)1 << 20;  // rows per streamed chunk of the IVF builds

// per-scan scratch of the exact 32-query scan, created with the index (sized for KNN_NQ_MAX queries, grid = n_cu workgroups,
// k <= KNNX_MAX_K_FAST)
struct FlatScratch {
  DevBuf<_Float16> qfrag;
  DevBuf<float> q_dev;  // [KNN_RQ_MAX, d]
  DevBuf<int> thr_g;
  DevBuf<float> part_s;
  DevBuf<uint32_t> part_i;
  DevBuf<int> part_n;
  DevBuf<float> D_dev;    // [KNN_RQ_MAX, KNNX_MAX_K_FAST]
  DevBuf<int64_t> I_dev;  // [KNN_RQ_MAX, KNNX_MAX_K_FAST]
  DevBuf<unsigned> range_cnt;  // [KNN_NQ] hit counters of a range scan
  DevBuf<int> maxnorm;    // largest row norm (order-encoded)
  DevBuf<unsigned long long> stats;  // device counters: [0] queries served by a proof-based path, [1] proofs that failed
  hipError_t alloc(int d, size_t G) {
    hipError_t e = hipSuccess;
    dev_alloc(e, qfrag, (size_t)d * 64);
    dev_alloc(e, q_dev, (size_t)KNN_RQ_MAX * d);
    dev_alloc(e, thr_g, KNN_NQ_MAX);
    dev_alloc(e, part_s, G * KNN_NQ_MAX * KNNX_MAX_K_FAST);
    dev_alloc(e, part_i, G * KNN_NQ_MAX * KNNX_MAX_K_FAST);
    dev_alloc(e, part_n, G * KNN_NQ_MAX);
    dev_alloc(e, D_dev, (size_t)KNN_RQ_MAX * KNNX_MAX_K_FAST);
    dev_alloc(e, I_dev, (size_t)KNN_RQ_MAX * KNNX_MAX_K_FAST);
    dev_alloc(e, range_cnt, KNN_NQ);
    dev_alloc(e, maxnorm, 1);
    if (e == hipSuccess) e = hipMemset(maxnorm, 0, sizeof(int));  // order-encoded +0.0f
    dev_alloc(e, stats, 2);
    if (e == hipSuccess) e = hipMemset(stats, 0, 2 * sizeof(unsigned long long));
    if (e != hipSuccess) *this = FlatScratch();
    return e;
  }
};

// wide scan (64 queries per pass): candidates, fallback results, proof flags; created with the index.
// Unproven queries of the proof-based scans (wide / RQ / int8) get the exact 32-query scan of their group.  On the device-buffer
// entry point that scan is launched for every group, gated on the device (no host round trip); the host-buffer entry points
// (search_fast_locked) read the gates back with the results instead and launch it only for a group that needs it -- 4 gated
// no-op kernels per group, 32 per 256-query batch, ~0.16 ms of launch slots (profiles/r06r_knn_b256_timeline.log).
struct WideScratch {
  DevBuf<int64_t> cand;   // [64, 64]
  DevBuf<float> approx;   // [64, 64]
  DevBuf<unsigned> need;  // [64]
  DevBuf<unsigned> gate;  // [2]
  DevBuf<float> Dfb;      // [32, 64]
  DevBuf<int64_t> Ifb;
  hipError_t alloc() {
    hipError_t e = hipSuccess;
    dev_alloc(e, cand, (size_t)KNN_NQ_MAX * KNN_WIDE_KW);
    dev_alloc(e, approx, (size_t)KNN_NQ_MAX * KNN_WIDE_KW);
    dev_alloc(e, need, KNN_NQ_MAX);
    dev_alloc(e, gate, 2);
    dev_alloc(e, Dfb, (size_t)KNN_NQ * KNNX_MAX_K_FAST);
    dev_alloc(e, Ifb, (size_t)KNN_NQ * KNNX_MAX_K_FAST);
    if (e != hipSuccess) *this = WideScratch();
    return e;
  }
};

// RQ scan (register-stationary queries, up to 256 per pass; knn_rq_kernels.hip): allocated on first use
struct RqScratch {
  DevBuf<_Float16> qfrag;  // [8 blocks][d/16][64][8]
  DevBuf<float> thr;       // [256]
  DevBuf<unsigned> cnt, lost, need, gate;  // [256] x3, [8]
  DevBuf<int> cntc;        // [256]
  DevBuf<float> hit_s;     // [256, KNN_RQ_CAP]
  DevBuf<uint32_t> hit_r;
  DevBuf<float> samp;      // [256, 64] sample scores
  DevBuf<int64_t> samp_i;
  DevBuf<_Float16> m_qfrag;  // fragment images of the sample scans of one batch, side by side (blocks of one launch)
  DevBuf<int> m_thr;       // [256] their global thresholds
  hipError_t alloc(int d) {
    if (qfrag) return hipSuccess;
    const size_t Q = KNN_RQ_MAX;
    hipError_t e = hipSuccess;
    dev_alloc(e, qfrag, (size_t)(Q / 32) * (d / 16) * 64 * 8);
    dev_alloc(e, thr, Q);
    dev_alloc(e, cnt, Q);
    dev_alloc(e, lost, Q);
    dev_alloc(e, need, Q);
    dev_alloc(e, gate, 8);
    dev_alloc(e, cntc, Q);
    dev_alloc(e, hit_s, Q * KNN_RQ_CAP);
    dev_alloc(e, hit_r, Q * KNN_RQ_CAP);
    dev_alloc(e, samp, Q * KNN_WIDE_KW);
    dev_alloc(e, samp_i, Q * KNN_WIDE_KW);
    dev_alloc(e, m_qfrag, (Q / KNN_NQ) * (size_t)d * 64);
    dev_alloc(e, m_thr, Q);
    if (e != hipSuccess) *this = RqScratch();
    return e;
  }
};

// int8 first stage of the flat scans (knn_rq_kernels.hip): the copy of the rows, allocated and built on first use, rebuilt after
// the rows change.  The image may be PARTIAL (KNNX_I8_MAX_BYTES, or what fits next to the fp16 rows): the other rows are scanned in fp16.
struct I8Copy {
  bool valid = false;          // rows / i8q.colscale / i8q.ab describe the current rows
  int64_t cap_rows = 0;
  int64_t nrows = 0;           // rows [0, nrows) are quantised with the current column scales (add() appends: only the new rows are done)
  int64_t scale_rows = 0;      // rows the column scales were taken over (a full rebuild once the index has doubled since)
  int planes = 1;              // int8 planes of a query: 2 when the column scales differ widely (decided at every full build)
  I8Dom dom;                   // dominant columns of the index (knn_kernels.h), decided with the planes
  DevBuf<int8_t> rows;         // tile-ordered image of rows [0, nrows) (knn_i8_quant_kernel): cap_rows / 32 tiles of 32 d bytes
  unsigned long long served = 0;       // queries answered through the int8 path (knnx_i8_active reports it)
  unsigned long long rest_served = 0;  // queries whose pass ran over an int8 part AND an fp16 rest
  // give the image back (it is an accelerator, not data: see malloc_or_reclaim)
  void release() {
    rows.reset();
    cap_rows = 0;
    nrows = 0;
    valid = false;
  }
};
// column statistics of the int8 copy and the query scratch of its pass: allocated on first use
struct I8Scratch {
  DevBuf<float> colscale;      // [d]
  DevBuf<int> colmax, ab;      // [d] (encoded), [2] (encoded A, B)
  DevBuf<int8_t> qdom;         // [2][256][4] the queries' 14-bit digits at the dominant positions (knn_i8_prep_kernel)
  DevBuf<int8_t> qfrag;        // [16 blocks][d / 64][64][16]
  DevBuf<int> thr;             // [256]
  DevBuf<float> lb;            // [256]
  DevBuf<float> hit_s;         // [256, KNN_I8_CAP]
  DevBuf<uint32_t> hit_r;
  hipError_t alloc(int d) {
    if (colscale) return hipSuccess;
    const size_t Q = KNN_RQ_MAX;
    hipError_t e = hipSuccess;
    dev_alloc(e, colscale, d);
    dev_alloc(e, colmax, d);
    dev_alloc(e, ab, 2);
    dev_alloc(e, qfrag, 2 * Q * d);
    dev_alloc(e, qdom, 2 * Q * 4);
    dev_alloc(e, thr, Q);
    dev_alloc(e, lb, Q);
    dev_alloc(e, hit_s, Q * KNN_I8_CAP);
    dev_alloc(e, hit_r, Q * KNN_I8_CAP);
    if (e != hipSuccess) *this = I8Scratch();
    return e;
  }
};

// IVF layout (ivf_layout_alloc, knnx_ivf.hip): rows -- or PQ codes -- live list-sorted and tile-padded in the arena; see knn_kernels.hip
struct IvfLayout {
  DevBuf<unsigned> tile0, ntile, size;  // [nlist] first tile, tiles, rows of a list
  DevBuf<int64_t> idmap;   // padded arena row -> id (-1 on pad rows)
  DevBuf<uint32_t> inv;    // id - id_base -> padded arena row
};
// single-block IVF scan (ivf_build_worklist): the work list of <= 32 queries; allocated with the layout
struct IvfScratch {
  DevBuf<unsigned> masks, off, nwork;  // [nlist] query mask of a list; off: unused since the atomic work list; [1] tiles in `work`
  DevBuf<uint4> work;      // [tiles of the arena]
  DevBuf<int64_t> Ic;      // [KNN_NQ, KNNX_MAX_K_FAST] coarse result
  DevBuf<float> Dc;
  DevBuf<float> scores;    // [KNN_NQ, nlist] coarse scores (nprobe > 64 only; allocated on first use)
};
// multi-block pass (scan_topk_ivf_multi): up to IVFM_BLK blocks of 32 queries in ONE coarse scan + ONE list scan; allocated on
// first use
struct IvfMultiScratch {
  DevBuf<_Float16> qfrag;      // [IVFM_BLK][d * 64] fragment images
  DevBuf<int> thr_c, thr_f;    // [32 IVFM_BLK] thresholds of the coarse / the list scan
  DevBuf<unsigned> nwork;      // 16 counters (8: union tiles) + masks [IVFM_BLK][nlist] behind them: one memset clears both
                               // (knn_kernels.hip launch_ivf_worklist*)
  unsigned* masks = nullptr;   // = nwork + 16 (not an allocation of its own)
  DevBuf<unsigned> off;        // unused since the atomic work list
  DevBuf<uint4> work;          // [IVFM_BLK][stride]
  unsigned stride = 0;
  DevBuf<float> scores;        // [32 IVFM_BLK, nlist] coarse scores of one pass
  hipError_t alloc(int d, size_t nl, int64_t capacity) {
    if (qfrag) return hipSuccess;
    const size_t tiles = (size_t)std::max<int64_t>(capacity / 32, 1);
    hipError_t e = hipSuccess;
    dev_alloc(e, qfrag, (size_t)IVFM_BLK * d * 64);
    dev_alloc(e, thr_c, (size_t)IVFM_BLK * 32);
    dev_alloc(e, thr_f, (size_t)IVFM_BLK * 32);
    dev_alloc(e, nwork, (size_t)IVFM_BLK * nl + 16);
    dev_alloc(e, off, (size_t)IVFM_BLK * nl);
    dev_alloc(e, work, (size_t)IVFM_BLK * tiles);
    dev_alloc(e, scores, (size_t)IVFM_BLK * 32 * nl);
    if (e != hipSuccess) {
      *this = IvfMultiScratch();
      return e;
    }
    masks = nwork + 16;
    stride = (unsigned)tiles;
    return e;
  }
};

// streaming build (knnx_ivf_begin .. knnx_ivf_end)
struct IvfBuild {
  int nlist = 0;
  int64_t total = 0, added = 0;
  std::vector<uint16_t> cent;
  // device staging of one chunk
  DevBuf<_Float16> rows;  // [IVFB_CHUNK, d] (knnx_ivfpq_add_codes stages its code bytes here: M <= 2 d)
  DevBuf<_Float16> rot;   // [IVFB_CHUNK, d_out] the chunk rotated, what the encoder reads (IVF-PQ with a rotation only)
  DevBuf<int64_t> ids;
  DevBuf<int32_t> lists, pos;
  // host mirror of the layout, so that every (list, position) a caller hands over is checked before it is scattered
  // (a position past its list, or used twice, would silently overwrite a neighbouring list's rows)
  std::vector<uint32_t> size, fill, tile0;
  std::vector<uint64_t> taken;  // one bit per padded arena row
};

// threshold mode of a compressed index's list scan (IVF-PQ: the ADC scan, IVF-SQ8: the code scan): the switch, the counters of
// knnx_ivf{pq,sq}_threshold_stats, and the device scratch of one threshold pass (allocated by the first one).  One per family.
struct ThrState {
  bool on = false;  // knnx_ivf{pq,sq}_set_threshold_scan: k > 64 and range_search are served; off: they are refused
  // since the index was created: queries served with k > 64, threshold scans launched (one launch serves a whole group), scans summed
  // over the queries that took part in them, hits fetched to the host
  int64_t queries = 0, scans = 0, query_scans = 0, hits = 0;
  DevBuf<float> tthr;       // [256] the per-query thresholds of one scan
  DevBuf<unsigned> tcnt;    // [256] its hit counters
  DevBuf<unsigned> tfetch;  // [256] tcnt with the queries that are not fetched set to 0 (range_fetch reads its counts on the device)
  hipError_t alloc() {
    if (tthr) return hipSuccess;
    hipError_t e = hipSuccess;
    dev_alloc(e, tthr, PQ_PASS);
    dev_alloc(e, tcnt, PQ_PASS);
    dev_alloc(e, tfetch, PQ_PASS);
    if (e != hipSuccess) tthr.reset(), tcnt.reset(), tfetch.reset();
    return e;
  }
};

// IVF-PQ (knnx_ivfpq_set_quantizer before knnx_ivf_begin; knn_pq_kernels.hip): the arena holds M code bytes per row, list-sorted
// and tile-padded like the IVF-Flat rows (`rows` stays null); the coarse quantiser is the IVF one
struct PqData {
  int m = 0;
  // the quantiser width d_out (knnx_ivfpq_set_out_dim; 0: none was given, the index has ONE width d).  With it the index has two:
  // knnx_index::d is what the user sees (queries, rows entering the build, the refine store, reconstruct), dq is where the centroids,
  // residuals, codebooks, lookup tables and codes live; the rotation A [dq][d] leads from one to the other.  Read it through pq_dq().
  int dq = 0;
  DevBuf<float> cb;                      // [M][256][d_out / M]
  DevBuf<uint8_t> codes;                 // [capacity][M]
  DevBuf<_Float16> bcent;                // centroids during the build (knnx_ivf_begin .. knnx_ivf_end)
  std::vector<unsigned> tile0_h, size_h; // host copy of the layout (knnx_ivfpq_get_codes)
  // OPQ rotation (knnx_ivfpq_set_rotation; empty: none): y = A x in front of everything above
  std::vector<float> rot_h;              // A, f32 [d_out][d] (knnx_ivfpq_get_rotation, knnx_shards_adopt)
  DevBuf<float> rot;                     // the same on the device (queries, back-rotation)
  DevBuf<_Float16> rot_w;                // [2 d_out][d] hi / lo tile image (row rotation of the build; released by knnx_ivf_end)
  // refine store (knnx_ivfpq_set_refine): the fp16 rows as they entered the build, un-rotated, in the arena order of the codes.
  // They live in knnx_index::rows ([capacity][d], allocated by knnx_ivf_begin); ivf.idmap / ivf.inv serve codes and rows alike.
  bool refine = false;
  int k_factor = 1;                      // candidates per result of a refine search (knnx_ivfpq_set_k_factor)
  ThrState thr;                          // threshold mode of the ADC scan
  // M = 256 (the two-half ADC scan, knnx_pq_plan.h): the budget of the partial-sum buffer (KNNX_PQ_PARTIAL_MAX_BYTES, read by
  // knnx_ivfpq_set_quantizer) and the slab width S of slab_np probed lists (host arithmetic on size_h, no device round trip: by the
  // first pass after the index is finished, and again by the first pass after nprobe changed; slab_np = 0: not computed)
  uint64_t partial_budget = 0, slab = 0;
  int slab_np = 0;
};
// one IVF-PQ search pass of up to PQ_PASS queries, allocated on first use
struct PqScratch {
  DevBuf<_Float16> qfrag;
  DevBuf<int> thr;          // [2][256] thresholds reset by the query prep (the coarse dump does not use them)
  DevBuf<float> scores;     // [256][nlist] coarse scores
  DevBuf<unsigned> masks;   // [8][nlist]
  DevBuf<unsigned> pcnt;    // [256]
  DevBuf<int> probe;        // [256][np_cap] probed lists
  DevBuf<float> pscore;     // [256][np_cap] their coarse scores
  int np_cap = 0;
  int np = 0;               // lists probed per query by the pass whose front half is in here (pq_front)
  DevBuf<float> lut;        // [256][M][256]
  DevBuf<float> part_s;     // [PQ_SLOTS][64] per-workgroup top-k of the ADC scan
  DevBuf<uint32_t> part_i;
  DevBuf<int> part_n;       // [PQ_SLOTS]
  DevBuf<float> qrot;       // [256][d_out] the rotated queries (allocated by scan_topk_pq when the index has a rotation)
  // refine (allocated by the first refine search): candidates of one pass and their exact scores, the partial lists of the candidate
  // scan for kc > 64, the ADC scores the merge writes next to the candidate ids for kc <= 64
  DevBuf<int64_t> rcand;    // [256][PQ_REFINE_MAX]
  DevBuf<float> rscore;     // [256][PQ_REFINE_MAX]
  DevBuf<float> rpart_s;    // [PQ_SLOTS][PQ_REFINE_MAX]
  DevBuf<uint32_t> rpart_r;
  DevBuf<float> rdc;        // [256][64]
  // M = 256 only (the two-half ADC scan): the row offset of every probe in its query's slab, written by pq_front; the partial sums
  // of the sub-group being scored, allocated on first use (knnx_ivfpq.hip: pq_half_buffer).  half_nq = n > 0: the buffer holds the
  // sums of all n queries of the pass whose front half is in here (one sub-group) -- cleared by pq_front, so they never outlive it.
  DevBuf<unsigned> poff;    // [256][np_cap]
  DevBuf<float> half;       // [g][S]
  uint64_t half_cap = 0;    // floats in half
  int half_nq = 0;
  hipError_t alloc_refine() {
    if (rcand) return hipSuccess;
    hipError_t e = hipSuccess;
    dev_alloc(e, rcand, (size_t)PQ_PASS * PQ_REFINE_MAX);
    dev_alloc(e, rscore, (size_t)PQ_PASS * PQ_REFINE_MAX);
    dev_alloc(e, rpart_s, (size_t)PQ_SLOTS * PQ_REFINE_MAX);
    dev_alloc(e, rpart_r, (size_t)PQ_SLOTS * PQ_REFINE_MAX);
    dev_alloc(e, rdc, (size_t)PQ_PASS * KNNX_MAX_K_FAST);
    if (e != hipSuccess) rcand.reset(), rscore.reset(), rpart_s.reset(), rpart_r.reset(), rdc.reset();
    return e;
  }
  // (a larger nprobe than any before regrows probe / pscore only)
  hipError_t alloc(int d, size_t nl, int m, int np) {
    if (qfrag && np <= np_cap) return hipSuccess;
    hipError_t e = hipSuccess;
    if (!qfrag) {
      dev_alloc(e, qfrag, (size_t)IVFM_BLK * d * 64);
      dev_alloc(e, thr, 2 * PQ_PASS);
      dev_alloc(e, scores, PQ_PASS * nl);
      dev_alloc(e, masks, IVFM_BLK * nl);
      dev_alloc(e, pcnt, PQ_PASS);
      dev_alloc(e, lut, (size_t)PQ_PASS * m * 256);
      dev_alloc(e, part_s, (size_t)PQ_SLOTS * KNNX_MAX_K_FAST);
      dev_alloc(e, part_i, (size_t)PQ_SLOTS * KNNX_MAX_K_FAST);
      dev_alloc(e, part_n, PQ_SLOTS);
    }
    dev_alloc(e, probe, (size_t)PQ_PASS * np);
    dev_alloc(e, pscore, (size_t)PQ_PASS * np);
    if (m == 256) dev_alloc(e, poff, (size_t)PQ_PASS * np);
    if (e != hipSuccess) *this = PqScratch();
    else np_cap = np;
    return e;
  }
};

// IVF-SQ8 (knnx_ivfsq_set_quantizer before knnx_ivf_begin; knn_sq_kernels.hip, knnx_ivfsq.hip): the arena holds d code bytes per row,
// list-sorted and tile-padded like the IVF-Flat rows (`rows` stays null); layout, coarse quantiser and probe rule are the IVF ones
struct SqData {
  bool on = false;
  std::vector<float> vmin_h, vdiff_h;    // the quantiser as it was given (knnx_ivfsq_get_quantizer, knnx_shards_adopt)
  DevBuf<float> vmin, scale, step;       // [d]; scale = 255 / vdiff and step = vdiff / 255 from the host, 0 where vdiff == 0
  DevBuf<uint8_t> codes;                 // [capacity][d]
  std::vector<unsigned> tile0_h, size_h; // host copy of the layout (knnx_ivfsq_get_codes)
  ThrState thr;                          // threshold mode of the list scan
};
// one IVF-SQ8 pass of up to IVFM_BLK x 32 queries (next to IvfMultiScratch, which serves its coarse half); allocated on first use
struct SqScratch {
  DevBuf<float> u;         // [256][d] q * step, scaled, in the scan's column order
  DevBuf<_Float16> qfrag;  // [IVFM_BLK][d * 64] its fragment images
  DevBuf<float> bq, inv;   // [256] bias and inverse scale of every query
  DevBuf<unsigned long long> trows;   // [256] rows in every query's probed lists (threshold passes; allocated by the first one)
  hipError_t alloc(int d) {
    if (u) return hipSuccess;
    hipError_t e = hipSuccess;
    dev_alloc(e, u, (size_t)IVFM_BLK * KNN_NQ * d);
    dev_alloc(e, qfrag, (size_t)IVFM_BLK * d * 64);
    dev_alloc(e, bq, (size_t)IVFM_BLK * KNN_NQ);
    dev_alloc(e, inv, (size_t)IVFM_BLK * KNN_NQ);
    if (e != hipSuccess) *this = SqScratch();
    return e;
  }
};

// list-ordered ids (knnx_ivf.hip: knnx_ivf_id_order / knnx_ivf_map_ids; include/knnx.h "List-ordered ids").  Empty until the first call.
// The layout it reads (ivf.tile0 / size / idmap / inv) does not change once the index is built, so this group has a mutex and a stream
// of its own: a translation on the request path never queues behind the scans that hold knnx_index::mu.
struct IdOrder {
  Stream stream;                  // (first: destroyed after the buffers below)
  std::mutex mu;
  bool ready = false;             // dense0 is built
  std::vector<int64_t> dense0_h;  // [nlist + 1] exclusive prefix sum of the list sizes
  DevBuf<int64_t> dense0;         // the same on the device
  // staging of knnx_ivf_map_ids, grown on demand up to one chunk (KNNX_ID_ORDER_CHUNK): a request's ids go in, their answers come back
  PinBuf pin;
  DevBuf<int64_t> dev;
  int64_t cap = 0;                // ids pin / dev hold
};

// what the most recent knnx_ivf_append* / knnx_ivf_merge_from that succeeded spent (knnx_grow.hip; knnx_ivf_grow_stats)
struct GrowStats {
  double assign_ms = 0, move_ms = 0, ids_ms = 0, fill_ms = 0;  // host time of the assignment pass; device time of the arena move, of its
                                                                // idmap / inv pass (part of move_ms), of the scatter / encode
  int64_t moved_bytes = 0;                          // payload bytes the move copied (occupied tiles of every arena)
  int64_t calls = 0;
};

// what the most recent knnx_ivf_remove_ids that succeeded spent (knnx_shrink.hip; knnx_ivf_remove_stats); a call that found nothing to
// remove counts, with zeros
struct ShrinkStats {
  double mark_ms = 0, plan_ms = 0, move_ms = 0, ids_ms = 0;  // device time of the phases (plan includes its host round trips)
  int64_t moved_bytes = 0;                                   // payload bytes of the survivors, every arena
  int64_t n_removed = 0;
  int64_t calls = 0;
};

// device post filter of one request (knnx_filter.hip: knnx_search_filtered; sizes: filter_sizes() of knnx_filter_plan.h).  Grow-only:
// alloc() keeps what it has when that is large enough, otherwise it replaces the WHOLE group by one sized for the request -- taking the
// int8 copy back (malloc_or_reclaim) before it gives up -- and leaves the group EMPTY when even that fails.  Used under knnx_index::mu.
struct FilterScratch {
  DevBuf<float> rows;         // [k_cap][d] the gathered result rows, normalised in place
  DevBuf<int64_t> ids;        // [k_cap]
  DevBuf<uint32_t> links;     // [FILTER_LINK_CAP] i << 16 | j
  DevBuf<int> counters;       // [FILTER_COUNTERS]
  DevBuf<float> vscores;      // [k_cap][v_cap] violence scores
  DevBuf<float> sscores;      // [k_cap][s_cap] safety scores
  DevBuf<uint8_t> drop;       // [k_cap]
  int k_cap = 0, v_cap = 0, s_cap = 0;
  hipError_t alloc(struct knnx_index* ix, int k, int v_out, int s_out);  // (defined below malloc_or_reclaim)
};

// hit pools of the range scans, grown on demand (knnx_range.hip: range_pool_alloc)
struct RangePools {
  DevBuf<float> s;
  DevBuf<uint32_t> i;
  size_t pool = 0;  // entries in s / i, shared by the queries of one scan
};

// scan timing (knnx_profile_enable / knnx_profile_get): an event pair around every main scan launch while `on`
struct Profile {
  bool on = false;
  std::vector<std::pair<Event, Event>> events;  // recorded pairs, collected by knnx_profile_get
  std::pair<Event, Event> open;                 // between begin() and end()
  // begin() before the launch, end() after it; both do nothing unless `timed`
  hipError_t begin(bool timed, hipStream_t st) {
    if (!timed) return hipSuccess;
    open = std::pair<Event, Event>();
    hipError_t e = open.first.create();
    if (e == hipSuccess) e = open.second.create();
    if (e == hipSuccess) e = hipEventRecord(open.first, st);
    return e;
  }
  hipError_t end(bool timed, hipStream_t st) {
    if (!timed) return hipSuccess;
    hipError_t e = hipEventRecord(open.second, st);
    if (e == hipSuccess) events.push_back(std::move(open));
    return e;
  }
};

// Request coalescer ("knnx_search is re-entrant; internally a batching queue"): concurrent single-query callers
// (the werkzeug request threads of clip_back.py:1018) queue here; one of them -- the leader -- serves everything that queued
// while the GPU was busy, up to one scan's worth with the same k, in ONE pass over HBM, then hands the lead on.
struct Coalescer {
  bool on = true;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<struct CoReq*> q;
  bool leader = false;
  int64_t batches = 0, queries = 0, largest = 0;
  std::vector<float> qbuf, Dbuf;
  std::vector<int64_t> Ibuf;
};

struct knnx_index {
  int device = 0;
  int d = 0;
  int n_cu = 256;
  int64_t ntotal = 0;
  int64_t capacity = 0;
  int64_t id_base = 0;
  Stream stream;           // (first: destroyed after everything that may still be queued on it has been freed)
  DevBuf<_Float16> rows;   // [capacity, d]; borrowed after knnx_attach_device_f16
  std::mutex mu;

  // switches, read from the environment once (knnx_create)
  int nt_loads = 0;        // KNNX_NT=1
  int wide_ok = 1;         // KNNX_WIDE=0 disables
  int rq_ok = 1;           // KNNX_RQ=0 disables
  int64_t rq_min_rows = KNN_RQ_MIN_ROWS;  // KNNX_RQ_MIN_ROWS overrides (tests run the RQ path on small indexes)
  int rq_sample_grid = 0;  // workgroups of the threshold-sample scans (0: chosen from the sample size; KNNX_RQ_SAMPLE_GRID overrides)
  int i8_env_ok = 1;       // KNNX_I8=0 disables
  int i8_ok = 1;           // = i8_env_ok until the copy's memory cannot be had (knnx_reset tries again)
  int i8_planes_env = 0;   // KNNX_I8_PLANES=1|2 forces the choice (and switches the dominant-column form off)
  int i8_dom_off = 0;      // KNNX_I8_DOM=0: never use the dominant-column form (two planes instead)
  int64_t i8_budget = 0;   // KNNX_I8_MAX_BYTES: cap on the int8 image (0: none)
  int ivfm_ok = 1;         // KNNX_IVF_MULTI=0, or an allocation failed: the 32-queries-per-pass IVF path

  FlatScratch flat;
  WideScratch wide;
  RqScratch rq;
  I8Copy i8;
  I8Scratch i8q;
  RangePools range;
  FilterScratch filter;
  Profile prof;
  Coalescer co;

  // pinned staging for host<->device hand-over
  PinBuf pin;
  // device scratch of reconstruct / range_fetch, kept between calls (hipMalloc + hipFree per request cost more than a
  // small search: hipFree synchronises the device); grown on demand, released with the index.  Used under mu only.
  struct Slot {
    DevBuf<void> p;
    size_t bytes = 0;
  } scratch[9];

  // IVF-Flat / IVF-PQ state
  int ivf_nlist = 0, ivf_nprobe = 1;
  knnx_index* cent = nullptr;  // coarse quantiser: a flat index over the fp16 centroids
  IvfLayout ivf;
  IvfScratch ivf1;
  IvfMultiScratch ivfm;
  int ivfm_last_blk = 0;          // blocks of the most recent IVF scan (0: the single-block path) -- knnx_ivf_last_scan_tiles
  bool ivfm_union_valid = false;  // the most recent pass also counted the union of its lists (profiling was on)
  IvfBuild ivfb;
  PqData pq;
  PqScratch pqs;
  SqData sq;
  SqScratch sqs;
  IdOrder ido;
  GrowStats grow;
  ShrinkStats shrink;

  // a proof-based scan that skipped its fallback (see WideScratch) says so here: 1 = rq.need / rq.gate, 2 = wide.need / wide.gate
  bool defer_fb = false;
  int defer_kind = 0, defer_nq = 0;

  // scratch hand-over between streams: the per-handle scratch above is shared by every call, so each launch sequence
  // first waits for the event the previous sequence recorded, whichever stream that ran on
  Event ev_scratch;
  bool ev_valid = false;
};

// the width of the quantiser space of an IVF-PQ index: d unless knnx_ivfpq_set_out_dim gave another
inline int pq_dq(const knnx_index* ix) { return ix->pq.dq ? ix->pq.dq : ix->d; }

// What the threshold passes of the two compressed families differ in (pq_thr_pass(): knnx_ivfpq.hip, sq_thr_pass(): knnx_ivfsq.hip);
// knnx_range.hip drives either through this table.  A pass is one front half over <= pass_max queries already in HBM, then the
// k = 64 scan, the probed-row totals and any number of threshold scans over what the front half left in the family's scratch.
struct ThrPass {
  const char* family;                        // "IVF-PQ" / "IVF-SQ8", for the messages
  bool (*is)(const knnx_index* ix);          // the index belongs to the family
  ThrState& (*thr)(knnx_index* ix);          // its threshold state
  int (*pass_max)(const knnx_index* ix);     // queries of one pass at most
  int (*front)(knnx_index* ix, const float* q_dev, int nq, hipStream_t st);
  // the top-64 scores of the pass -> D64 host [nq][64], -FLT_MAX padded.  Synchronises.
  int (*top64)(knnx_index* ix, int nq, float* D64, hipStream_t st);
  // rows in the probed lists of every query of the pass -> total [nq].  Synchronises.
  int (*probed_rows)(knnx_index* ix, int nq, std::vector<int64_t>& total, hipStream_t st);
  // the threshold kernel(s) alone: thresholds thr.tthr [nq] (+INFINITY: a finished query) -> exact counts in thr.tcnt, hits in
  // ix->range at q * cap
  int (*launch_threshold)(knnx_index* ix, int nq, unsigned cap, hipStream_t st);
};

// ---- what one host file calls in another ---------------------------------------------------------
// knnx_api.hip
int set_dev(const knnx_index* ix);
int ensure_pin(knnx_index* ix, size_t bytes);
int ensure_scratch(knnx_index* ix, int slot, size_t bytes, void** out);
int scratch_acquire(knnx_index* ix, hipStream_t st);
int scratch_release(knnx_index* ix, hipStream_t st);
int scan_cap(int d, int k);
int scan_topk(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st,
              const unsigned* gate = nullptr);
int search_fast_locked(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I);
// knnx_range.hip
int search_large_k_locked(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I);
int search_large_k_thr_locked(knnx_index* ix, const ThrPass& P, const float* q, int n, int k, float* D, int64_t* I);
int thr_set_switch(knnx_index* ix, const ThrPass& P, int on);
int thr_switch(const knnx_index* ix, const ThrPass& P);
int thr_stats(knnx_index* ix, const ThrPass& P, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits);
// knnx_ivf.hip
int ivf_build_worklist(knnx_index* ix, const float* q_dev, int nq, hipStream_t st, const unsigned* gate);
bool ivfm_usable(const knnx_index* ix, int nq, int k);
int ivfm_alloc(knnx_index* ix);
int ivfm_coarse_worklists(knnx_index* ix, const float* q_dev, int nq, int nblk, int grid, int* thr_f_or_null, hipStream_t st);
int scan_topk_ivf_multi(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st);
int ivf_import_codes_locked(knnx_index* ix, uint8_t* arena, int width, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists,
                            const int32_t* pos);
int ivf_export_codes_locked(knnx_index* ix, const uint8_t* arena, int width, const std::vector<unsigned>& tile0_h,
                            const std::vector<unsigned>& size_h, const char* family, int64_t* ids, int32_t* lists, uint8_t* codes);
// knnx_grow.hip: the one place where a layout built next to the index is swapped in and every cache of the old one dropped
int ivf_swap_in(knnx_index* ix, IvfLayout& L, DevBuf<uint4>& work, DevBuf<uint8_t>& pq_codes, DevBuf<uint8_t>& sq_codes, DevBuf<_Float16>& rows,
                const std::vector<unsigned>& tile0_h, const std::vector<unsigned>& size_h, int64_t prow, int64_t ntotal);
// knnx_ivfpq.hip
int scan_topk_pq(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st);
const ThrPass& pq_thr_pass();
// decoded rows of n ids (device) -> out f32 [n][d] in the ORIGINAL space (back-rotated when the index has a rotation; scratch slot 5);
// on an index with a refine store: the stored rows themselves
int pq_decode_rows(knnx_index* ix, const int64_t* ids_dev, int64_t n, float* out_dev, hipStream_t st);

// knnx_ivfsq.hip
int scan_topk_sq(knnx_index* ix, const float* q_dev, int nq, int k, float* D_out, int64_t* I_out, hipStream_t st);
// queries of one IVF-SQ8 pass: IVFM_BLK blocks of 32, fewer where KNNX_GRID leaves fewer workgroups than blocks
inline int sq_pass_max(const knnx_index* ix) { return KNN_NQ * std::max(1, std::min(IVFM_BLK, ix->n_cu)); }
const ThrPass& sq_thr_pass();
// decoded rows of n ids (device) -> out f32 [n][d]; -1 -> 0xFF bytes
int sq_decode_rows(knnx_index* ix, const int64_t* ids_dev, int64_t n, float* out_dev, hipStream_t st);

// the int8 copy is an accelerator, not data: whoever needs device memory and cannot get it takes the copy's back and tries once more
// (the lazily built copy must not starve the range pools / large-k scratch that fitted before it existed)
template <class T>
inline hipError_t malloc_or_reclaim(knnx_index* ix, DevBuf<T>& b, size_t n) {
  hipError_t e = b.alloc(n);
  if (e != hipSuccess && ix->i8.rows) {
    (void)hipGetLastError();
    ix->i8.release();
    ix->i8_ok = 0;  // it did not fit next to what the index needs: do not rebuild it on the next search
    e = b.alloc(n);
  }
  return e;
}

inline hipError_t FilterScratch::alloc(knnx_index* ix, int k, int v_out, int s_out) {
  if (rows && k <= k_cap && v_out <= v_cap && s_out <= s_cap) return hipSuccess;
  const int kc = std::max(k, k_cap), vc = std::max(v_out, v_cap), sc = std::max(s_out, s_cap);
  const FilterSizes z = filter_sizes(kc, ix->d, vc, sc);
  *this = FilterScratch();  // (the old buffers go first: the new group need not fit next to them)
  hipError_t e = malloc_or_reclaim(ix, rows, z.rows);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, ids, z.ids);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, links, z.links);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, counters, z.counters);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, vscores, z.vscores);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, sscores, z.sscores);
  if (e == hipSuccess) e = malloc_or_reclaim(ix, drop, z.drop);
  if (e != hipSuccess) {
    *this = FilterScratch();
    return e;
  }
  k_cap = kc, v_cap = vc, s_cap = sc;
  return hipSuccess;
}

// postfilter.hip (the MLP handle is its own object with its own mutex; these two are what the filter asks of it)
void knnx_mlp_shape(const knnx_mlp* m, int* d_in, int* d_out, int* n_layers, int* has_bias);
// knnx_api.hip: the dispatch of knnx_search for host buffers with ix->mu held (no coalescing, no reconstruct)
int search_locked(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I);

#pragma GCC visibility pop
