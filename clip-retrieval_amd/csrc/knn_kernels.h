// knn_kernels.h -- launchers of the gfx950 kNN kernels (internal; the public ABI is include/knnx.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace knnx {

constexpr int KNN_NQ = 32;     // query columns of one exact scan (MFMA N dimension)
constexpr int KNN_NQ_MAX = 64; // queries of one wide scan (two 32-column blocks, fp16-hi scores + exact re-scoring)
constexpr int KNN_WIDE_KW = 64;   // candidates per query the wide scan keeps
constexpr int KNN_WIDE_MAX_K = 48;  // largest k it serves (needs a gap between the k-th exact and the 64th approx score)
constexpr int KNN_WAVES = 8;   // waves per workgroup, one 32-row tile each
constexpr int KNN_WG = KNN_WAVES * 64;
constexpr float KNN_LO_SCALE = 2048.f;
constexpr float KNN_LO_INV = 1.f / 2048.f;
constexpr int KNN_LDS_BYTES = 160 * 1024;

struct ScanArgs {
  const _Float16* X;
  int64_t N;
  int d;
  const _Float16* qfrag;
  int nq;
  int k;
  int cap;
  int grid;
  int mode;  // 0 top-k, 1 range, 2 dump every score into range_s [nq, range_cap = N]
  int nt;    // 1 = nontemporal X loads (A/B switch, KNNX_NT=1)
  int* thr_g;
  float* part_s;
  uint32_t* part_i;
  int* part_n;
  float range_thr;
  unsigned* range_cnt;
  unsigned range_cap;
  float* range_s;
  uint32_t* range_i;
  // IVF: walk this work list of {tile, query mask, valid rows, -} items instead of all tiles (null = flat scan)
  const uint4* work;
  const unsigned* nwork;
  int wide;              // 1: QB = 2 wide scan (64 queries, approximate scores; flat top-k only)
  const unsigned* gate;  // run only if *gate != 0 (null: always)
  int tstride;           // flat scans: visit every tstride-th 32-row tile only (0 / 1 = all): the sample pass of the RQ scan
  // nblk > 1: blocks of 32 (wide: 64) queries side by side in ONE launch (modes 0 and 2; grid % nblk == 0): qfrag [nblk][d * 64],
  // thr_g [32 nblk] (wide: [64 nblk]), work [nblk][work_stride], nwork [nblk], part_* block-major (knn_kernels.hip: knn_scan_kernel)
  int nblk;
  unsigned work_stride;
};

size_t scan_smem_bytes(int d, int cap, int nq_slots);
hipError_t launch_prep(const float* q_dev, int nq, int d, _Float16* qfrag, int* thr_g, unsigned* range_cnt, int wide,
                       const unsigned* gate, hipStream_t st);
// (wide: blocks of 64 queries, the fp16-hi fragment images of the QB = 2 scan)
hipError_t launch_prep_blocks(const float* q_dev, int nq, int d, _Float16* qfrag, int* thr_a, int* thr_b_or_null, hipStream_t st, int wide = 0);
hipError_t launch_maxnorm(const _Float16* X, int64_t n, int d, int* maxnorm_enc, hipStream_t st);
hipError_t launch_rescore(const _Float16* X, int d, const float* q, const int64_t* cand, const float* approx, int nq, int kw,
                          int k, int64_t id_base, const int* maxnorm_enc, float* D, int64_t* I, unsigned* need, unsigned* gate,
                          unsigned long long* stats, hipStream_t st);
hipError_t launch_select(const unsigned* need, int q0, int nq, int k, const float* Dfb, const int64_t* Ifb, float* D, int64_t* I,
                         hipStream_t st);
hipError_t launch_scan(const ScanArgs& a, hipStream_t st);
hipError_t launch_merge_u32(const float* ps, const uint32_t* pi, const int* pn, int P, int nq_stride, int kin,
                            int nq, int k, int64_t id_base, const int64_t* idmap_or_null, float* D, int64_t* I,
                            const unsigned* gate_or_null, hipStream_t st, int blk_q = 0,  // blk_q = 32: block-major partial lists, or
                            const unsigned* blk_work = nullptr, int nblk = 0, int G = 0);  // (after a multi-block list scan of G
                            // workgroups) block b's lists are the slots of the workgroups that served it: P = upper bound (LDS size)
// IVF-Flat helpers (see knn_kernels.hip)
hipError_t launch_ivf_worklist(const int64_t* Ic, int nq, int nprobe, int nlist, unsigned* masks, const unsigned* tile0,
                               const unsigned* ntile, const unsigned* size, unsigned* off, uint4* work, unsigned* nwork,
                               hipStream_t st, unsigned work_stride = 0);
hipError_t launch_ivf_worklist_from_scores(const float* scores, int nq, int nprobe, int nlist, unsigned* masks, const unsigned* tile0,
                                           const unsigned* ntile, const unsigned* size, unsigned* off, uint4* work, unsigned* nwork,
                                           hipStream_t st, unsigned work_stride = 0);
hipError_t launch_ivf_union_tiles(const unsigned* masks, int nblk, int nlist, const unsigned* ntile, unsigned* out, hipStream_t st);
// the nprobe best lists of every query from a score dump [nq, nlist] -> bit q % 32 of masks[q / 32][l] (masks cleared first)
hipError_t launch_ivf_select_mark(const float* scores, int nq, int nprobe, int nlist, unsigned* masks, hipStream_t st);
hipError_t launch_ivf_relayout(const _Float16* src, _Float16* dst, int d, int nlist, const int64_t* src0, const unsigned* tile0,
                               const unsigned* ntile, const unsigned* size, const int64_t* ids, int64_t id_lo, int64_t n_ids,
                               int64_t* idmap, uint32_t* inv, hipStream_t st);
hipError_t launch_gather_inv(const _Float16* X, int d, int64_t id_lo, int64_t n_ids, const uint32_t* inv, const int64_t* ids,
                             int64_t n, float* out, hipStream_t st);
hipError_t launch_merge_i64(const float* ps, const int64_t* pi, int P, int nq, int kin, int k, float* D,
                            int64_t* I, hipStream_t st);
hipError_t launch_merge_sorted(const float* Dp, const int64_t* Ip, int P, int n, int k, float* D, int64_t* I, hipStream_t st);
hipError_t launch_gather(const _Float16* X, int64_t N, int d, int64_t id_base, const int64_t* ids, int64_t n,
                         float* out, hipStream_t st);
hipError_t launch_f32_to_f16(const float* in, _Float16* out, int64_t n, hipStream_t st);
hipError_t launch_range_sort(const float* rs, const uint32_t* ri, const unsigned* cnt, unsigned cap,
                             const int64_t* lims, int64_t id_base, const int64_t* idmap_or_null, int nq, float* D, int64_t* I,
                             hipStream_t st);
// hit lists longer than this are sorted by launch_range_sort_long (radix) instead of launch_range_sort (rank by counting)
constexpr unsigned RANGE_SORT_SMALL = 4096;
hipError_t launch_range_sort_long(const float* vs, const uint32_t* ri, unsigned n, int64_t id_base, const int64_t* idmap_or_null,
                                  int key_bits, uint32_t* k0, uint32_t* k1, float* v0, float* v1, unsigned* hist, float* D, int64_t* I,
                                  hipStream_t st);
hipError_t launch_synth(_Float16* X, int64_t row_begin, int64_t n, int d, uint64_t seed, hipStream_t st, int dominant = 0);
// the mixture corpus of BASELINE config 5 (knn_kernels.hip: knn_synth_mix_kernel): destination row i = corpus row
// row_begin + i * row_stride; P_table = synth_mix_table_bytes(d) bytes of device scratch
hipError_t launch_synth_mix(_Float16* X, int64_t row_begin, int64_t row_stride, int64_t n, int d, uint64_t seed, int64_t n_clusters,
                            short* P_table, hipStream_t st);
size_t synth_mix_table_bytes(int d);
hipError_t launch_copy_rows(const _Float16* src, int d, const int64_t* src_rows, const int32_t* dst_rows, int64_t n, _Float16* dst,
                            hipStream_t st);
hipError_t launch_ivf_hist(const int32_t* lists, int64_t n, int nlist, unsigned long long* hist, hipStream_t st);
// list-ordered ids (knn_idorder_kernels.hip; dense0 [nlist + 1] = exclusive prefix sum of the list sizes, knnx_id_order.h):
// out[t] = idmap[arena row of ordinal o0 + t], t < n -- a slice of new_to_old (prow: rows of the padded arena)
hipError_t launch_ivf_new_to_old(const int64_t* idmap, int64_t prow, const unsigned* tile0, const int64_t* dense0, int nlist, int64_t o0,
                                 int64_t n, int64_t* out, hipStream_t st);
// out[t] = id_base + ordinal of the row with id ids[t] (-1 -> -1; out may be ids); ids == null: the ids id_base + i0 + t, a slice of old_to_new
hipError_t launch_ivf_map_ids(const uint32_t* inv, int64_t id_base, int64_t ntotal, const unsigned* tile0, const int64_t* dense0, int nlist,
                              const int64_t* ids_or_null, int64_t i0, int64_t n, int64_t* out, hipStream_t st);
// the arena move of a growing index (knn_grow_kernels.hip; src_tile [tiles]: the old tile of every new tile or GROW_NO_TILE, knnx_grow_plan.h):
// dst tile t = src tile src_tile[t], or zeros; `width` bytes per arena row (a multiple of 16), tiles of 32 rows; src and dst distinct
hipError_t launch_ivf_grow_move(const void* src, void* dst, int width, const uint32_t* src_tile, int64_t tiles, int n_cu, hipStream_t st);
// ... and its ids: idmap [prow] = the old id of every moved row, -1 elsewhere; inv[id - id_lo] = the new arena row of every moved id
hipError_t launch_ivf_grow_ids(const int64_t* idmap_old, const uint32_t* src_tile, int64_t prow, int64_t id_lo, int64_t n_ids, int64_t* idmap,
                               uint32_t* inv, hipStream_t st);
// removing ids from a built index (knn_shrink_kernels.hip; the arithmetic is knnx_shrink_plan.h), in the order of a call.  dead and rank
// are allocated in whole blocks of SHRINK_BLOCK ids (dead zeroed), tmask / tpos have one entry per tile of the OLD arena.
hipError_t launch_ivf_shrink_mark(const int64_t* ids, int64_t m, int64_t id_lo, int64_t n, uint8_t* dead, hipStream_t st);
hipError_t launch_ivf_shrink_rank_sum(const uint8_t* dead, int64_t n, uint32_t* blocksum, hipStream_t st);
hipError_t launch_ivf_shrink_rank_apply(const uint8_t* dead, int64_t n, const uint32_t* blockoff, uint32_t* rank, hipStream_t st);
hipError_t launch_ivf_shrink_mask(const int64_t* idmap, int64_t prow, int64_t id_lo, int64_t n, const uint8_t* dead, uint32_t* tmask,
                                  hipStream_t st);
hipError_t launch_ivf_shrink_list_scan(const unsigned* tile0, const unsigned* ntile, int nlist, const uint32_t* tmask, uint32_t* tpos,
                                       unsigned* size_new, hipStream_t st);
// tpos -> dst0 in place, once the new layout is on the device
hipError_t launch_ivf_shrink_dst0(const unsigned* tile0_old, const unsigned* ntile_old, const unsigned* tile0_new, int nlist, uint32_t* tpos,
                                  hipStream_t st);
// the survivors of source tile t -> the run of `width`-byte rows at destination row dst0[t]; src and dst distinct
hipError_t launch_ivf_shrink_move(const void* src, void* dst, int width, const uint32_t* tmask, const uint32_t* dst0, int64_t tiles, int n_cu,
                                  hipStream_t st);
// zeros over the pad rows of every list of the NEW layout
hipError_t launch_ivf_shrink_pads(void* dst, int width, const unsigned* tile0, const unsigned* ntile, const unsigned* size, int nlist,
                                  hipStream_t st);
// idmap (already all -1) and inv of the new arena
hipError_t launch_ivf_shrink_ids(const int64_t* idmap_old, int64_t prow_old, int64_t id_lo, int64_t n, const uint32_t* tmask,
                                 const uint32_t* dst0, const uint32_t* rank, int64_t* idmap, uint32_t* inv, hipStream_t st);

// ---- register-stationary-queries (RQ) scan, knn_rq_kernels.hip: up to rq_queries_per_pass(d) queries per pass over HBM
constexpr int KNN_RQ_MAX = 256;        // queries of one RQ pass at d <= 768 (128 at d = 1024)
// The sample pass visits every S-th 32-row tile, S = min(1024, tiles / 4096) (>= 4096 tiles = 131 k rows sampled); the
// threshold is the J-th best sample score with J = k + 8 up to S = 128 and J = (k + 8) * 128 / S (>= 6) beyond, i.e. ~6 k
// expected hits per query whatever the index size.  The number of index rows above the J-th best of a 1/S sample is
// distribution-free (~ S * Gamma(J)): at J = 9, S = 763 (100 M rows) P(hits > 32768) < 1e-15 and P(hits < k) = 0.
// (A 1/128 sample of 100 M rows cost 0.9 ms per 64-query pass -- cold LDS queues are pruned every round -- 3.6 ms of a
// 45 ms search; the 1/763 sample 0.3 ms.)
constexpr int KNN_RQ_STRIDE = 1024;
constexpr int KNN_RQ_MARGIN = 8;
constexpr unsigned KNN_RQ_CAP = 32768; // hit list entries per query
constexpr int64_t KNN_RQ_MIN_ROWS = (int64_t)1 << 21;  // below this the 64-query scan is used
int rq_queries_per_pass(int d);  // 0: no RQ kernel for this d
hipError_t launch_rq_prep(const float* q_dev, int nq, int d, _Float16* qfrag, const float* samp, int kw, int J, float slack,
                          float* thr, unsigned* cnt, unsigned* lost, hipStream_t st);
hipError_t launch_rq_scan(const _Float16* X, int64_t N, int d, int nq, const _Float16* qfrag, const float* thr, unsigned* cnt,
                          unsigned cap, float* hit_s, uint32_t* hit_r, unsigned* lost, const unsigned* gate, int grid,
                          hipStream_t st, uint32_t row_off = 0);  // row_off: X is a slice starting at that row of the index (added to the hits' rows)
// IVF build (knn_rq_kernels.hip / knn_kernels.hip): out[i] = argmax_l <P[i], C[l]> (fp16 rows, exact fp32 scores, ties -> smaller l)
hipError_t launch_assign(const _Float16* C, int64_t nlist, int d, const _Float16* P, int64_t n, int32_t* out, hipStream_t st);
// one Lloyd update (spherical): cent[l] = fp16(unit-norm mean of X[order[off[l] .. off[l+1])]) (lists with no member keep their row); one workgroup per list
hipError_t launch_kmeans_update(const _Float16* X, int d, const int64_t* order, const int64_t* off, int nlist, _Float16* cent,
                                hipStream_t st);
// scatter n assigned rows into the tile-padded list-sorted arena: dst row = tile0[list] * 32 + pos; lays down idmap / inv
// (ids == null: row i carries id id0 + i)
hipError_t launch_ivf_scatter(const _Float16* src, int64_t n, int d, const int32_t* lists, const int32_t* pos, const int64_t* ids,
                              int64_t id0, const unsigned* tile0, int64_t id_lo, int64_t n_ids, _Float16* dst, int64_t* idmap,
                              uint32_t* inv, hipStream_t st);
hipError_t launch_rq_rescore(const _Float16* X, int d, const float* q, int nq, const unsigned* cnt, unsigned cap, float* hit_s,
                             const uint32_t* hit_r, int* cntc, hipStream_t st);
hipError_t launch_rq_proof(const float* q, int nq, int d, int k, const float* D, const float* thr, const unsigned* cnt,
                           unsigned cap, const unsigned* lost, const int* maxnorm, unsigned* need, unsigned* gate,
                           unsigned long long* stats, hipStream_t st);

// ---- int8 first stage of the flat scans (knn_rq_kernels.hip, "int8 first stage"): exact results from half the bytes
constexpr int KNN_I8_STRIDE = 32;          // the sample pass visits every S-th tile, S = min(this, tiles / 4096): threshold ~ rank (k + 8) S
constexpr unsigned KNN_I8_CAP = KNN_RQ_CAP;  // hit list entries per query (knn_merge_kernel holds a query's whole list in LDS: 32 768 x 4 B)
int i8_supported(int d);
// Dominant columns of an index: up to four columns whose scale is far above the others' sit in BYTES 0..3 of every row of
// the int8 image (a column permutation private to the image: position p of the image holds column p of the row, except the nfix
// positions listed here) and are left out of the int8 MFMA product; the scan adds their part with 14-bit query digits on the
// vector ALU (knn_rq8_scan_kernel, DOM).  n = 0: no dominant columns, the image is in column order.
struct I8Dom {
  int n = 0;     // dominant columns = positions 0 .. n - 1
  int nfix = 0;  // positions whose column is not the position
  int pos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int src[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
hipError_t launch_i8_scales(const _Float16* X, int64_t N, int d, int* colmax_enc, float* colscale, int* ab_enc, hipStream_t st);
hipError_t launch_i8_quant(const _Float16* X, int64_t N, int64_t row_from, int64_t row_to, int d, const float* colscale, const I8Dom& dom,
                           int8_t* X8, int* ab_enc, hipStream_t st);
hipError_t launch_i8_prep(const float* q_dev, int nq, int d, const float* colscale, const I8Dom& dom, const int* ab_enc, const int* maxnorm,
                          const float* samp, int kw, int J, int planes, int refine, int8_t* qfrag8, int8_t* qdom, int* thr_i, float* thr_lb,
                          float* thr_rest, unsigned* cnt, unsigned* lost, hipStream_t st);
hipError_t launch_rq8_scan(const int8_t* X8, int64_t N, int d, int nq, int planes, const int8_t* qfrag8, const int8_t* qdom, const int* thr_i,
                           unsigned* cnt, unsigned cap, float* hit_s, uint32_t* hit_r, unsigned* lost, int grid, int tstep, hipStream_t st);
hipError_t launch_i8_proof(int nq, int k, const float* D, const float* thr_lb, const unsigned* cnt, unsigned cap, const unsigned* lost,
                           unsigned* need, unsigned* gate, unsigned long long* stats, hipStream_t st);

// ---- IVF-PQ (knn_pq_kernels.hip): faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), inner product, by_residual
constexpr int PQ_MAX_K = 64;  // k of the ADC scan's candidate queues
bool pq_supported(int d, int M);  // M in {16, 32, 64, 128}, M | d, d / M <= 64; or M = 256 with d in {512, 768, 1024}
// codes[row * M + m] = argmin_j ||r_m - cb[m][j]||^2, r = f32(X[i]) - f32(cent[lists[i]]); row = tile0[lists[i]] * 32 + pos[i] (tile0 == null:
// row = i); idmap != null: also idmap[row] = id (ids[i], or id0 + i) and inv[id - id_lo] = row
hipError_t launch_pq_encode(const _Float16* X, int64_t n, int d, int M, const int32_t* lists, const _Float16* cent, const float* cb,
                            const unsigned* tile0, const int32_t* pos, const int64_t* ids, int64_t id0, int64_t id_lo, int64_t n_ids,
                            uint8_t* codes, int64_t* idmap, uint32_t* inv, hipStream_t st);
// one Lloyd update of the codebooks from the sample: order [M][n] (members of each (m, j), ascending row), off [M][257]
hipError_t launch_pq_update(const _Float16* X, int d, int M, const int32_t* lists, const _Float16* cent, const int32_t* order,
                            const int32_t* off, int64_t n, float* cb, hipStream_t st);
hipError_t launch_pq_seed(const _Float16* X, int d, int M, const int32_t* lists, const _Float16* cent, const int32_t* mj, const int64_t* rows,
                          int64_t n, float* cb, hipStream_t st);
hipError_t launch_pq_lut(const float* q, int nq, int d, int M, const float* cb, float* lut, hipStream_t st);
hipError_t launch_pq_probe(const unsigned* masks, const float* scores, int nq, int nlist, int np, unsigned* pcnt, int* probe, float* pscore,
                           hipStream_t st);
size_t pq_scan_smem_bytes(int M);
hipError_t launch_pq_adc_scan(const uint8_t* codes, int M, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt,
                              int np, int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int k, int nq,
                              float* part_s, uint32_t* part_i, int* part_n, hipStream_t st);
hipError_t launch_pq_decode(const uint8_t* codes, int d, int M, const float* cb, const _Float16* cent, const unsigned* tile0, int nlist,
                            int64_t id_lo, int64_t n_ids, const uint32_t* inv, const int64_t* ids, int64_t n, float* out, hipStream_t st);
// Refine (faiss IndexRefineFlat(IndexIVFPQ)): kc = k x k_factor candidates by ADC score, re-scored from the fp16 rows.
constexpr int PQ_REFINE_MAX = 512;   // largest kc
constexpr int PQ_SEL_MAX = 16384;    // entries (shares x kc) the cross-share selection sorts in the LDS: 128 KiB
// the ADC scan for 64 < kc <= PQ_REFINE_MAX: partial list s * nq + q of part_s / part_r / part_n holds <= kc (score, arena row) entries
hipError_t launch_pq_cand_scan(const uint8_t* codes, int M, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt,
                               int np, int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int kc, int nq,
                               float* part_s, uint32_t* part_r, int* part_n, hipStream_t st);
// ... and the ids of the best kc of every query's nsplit lists (nsplit * kc <= PQ_SEL_MAX) -> cand [nq][kc], -1 padded, any order
hipError_t launch_pq_cand_select(const float* part_s, const uint32_t* part_r, const int* part_n, int nsplit, int nq, int kc,
                                 const int64_t* idmap, int64_t* cand, hipStream_t st);
// es[q][c] = <f32(X[inv[cand[q][c] - id_lo]]), q> (fixed summation order: knnx.h), then D / I = the top k of them, padded
hipError_t launch_pq_refine(const _Float16* X, int d, const float* q, int nq, int64_t id_lo, int64_t n_ids, const uint32_t* inv,
                            const int64_t* cand, int kc, int k, float* es, float* D, int64_t* I, hipStream_t st);
// the exact scores alone for any kc (the large-k refine search): es [nq][kc], -FLT_MAX where cand holds no id of the index
hipError_t launch_pq_rescore(const _Float16* X, int d, const float* q, int nq, int64_t id_lo, int64_t n_ids, const uint32_t* inv,
                             const int64_t* cand, int kc, float* es, hipStream_t st);
// Threshold mode of the ADC scan (pq_range_scan_kernel): every row of the probed lists with score > thr[q] (strict; +INFINITY: the
// query is skipped) is appended to hit_s / hit_r [q * cap ..] as (score, arena row); cnt[q] (cleared by the launcher) counts the hits
// exactly even when more than cap of them exist.  Scores are those of launch_pq_adc_scan, bit for bit.
hipError_t launch_pq_range_scan(const uint8_t* codes, int M, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt,
                                int np, int nsplit, const unsigned* tile0, const unsigned* size, const float* thr, unsigned* cnt,
                                unsigned cap, float* hit_s, uint32_t* hit_r, int nq, hipStream_t st);
// M = 256: the ADC stage in two halves of m (knn_pq_kernels.hip, above pq_probe_offsets_kernel).  poff [nq][np]: launch_pq_probe_offsets
// after launch_pq_probe.  The others serve queries q0 .. q0 + g - 1 of the pass's nq: launch_pq_adc_lower fills their slabs (half: g x
// slab floats; thr null or the thresholds of a threshold scan), the *_upper launchers are launch_pq_adc_scan / _cand_scan / _range_scan
// continued from those sums (launch_pq_range_upper does NOT clear cnt).
hipError_t launch_pq_probe_offsets(const int* probe, const unsigned* pcnt, int np, const unsigned* size, unsigned* poff, int nq, hipStream_t st);
hipError_t launch_pq_adc_lower(const uint8_t* codes, const float* lut, const int* probe, const unsigned* pcnt, int np, int nsplit,
                               const unsigned* tile0, const unsigned* size, const unsigned* poff, const float* thr, size_t slab, int q0, int g,
                               float* half, hipStream_t st);
hipError_t launch_pq_adc_upper(const uint8_t* codes, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt, int np,
                               int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int k, int nq, float* part_s,
                               uint32_t* part_i, int* part_n, const float* half, const unsigned* poff, size_t slab, int q0, int g,
                               hipStream_t st);
hipError_t launch_pq_cand_upper(const uint8_t* codes, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt, int np,
                                int nsplit, const unsigned* tile0, const unsigned* size, const int64_t* idmap, int kc, int nq, float* part_s,
                                uint32_t* part_r, int* part_n, const float* half, const unsigned* poff, size_t slab, int q0, int g,
                                hipStream_t st);
hipError_t launch_pq_range_upper(const uint8_t* codes, const float* lut, const int* probe, const float* pscore, const unsigned* pcnt, int np,
                                 int nsplit, const unsigned* tile0, const unsigned* size, const float* thr, unsigned* cnt, unsigned cap,
                                 float* hit_s, uint32_t* hit_r, const float* half, const unsigned* poff, size_t slab, int q0, int g,
                                 hipStream_t st);
// OPQ rotation in front of IVF-PQ (A f32 [d_out][d], y = A x; d <= d_out, both in {256, 512, 768, 1024}; d_out = d: the square
// rotation).  launch_rot_split: A -> W fp16 [2 d_out][d], the hi / lo tile image launch_rotate_f16 (knn_rq_kernels.hip, MFMA) streams:
// Y[i] = fp16(A P[i]) (P rows d wide, Y rows d_out wide), Y and P distinct.  launch_rot_queries: out[i] = A q[i] in fp32, d_out wide
// (nq <= 256 per launch is what it is sized for; any nq works).  launch_rot_back: out[i] = A^T dec[i] in fp32, dec d_out wide, out d wide
// (rows of 0xFF bytes stay 0xFF bytes; out and dec distinct).  launch_xty: G = X^T Y, f32 [d][d], fixed summation order.
hipError_t launch_rot_split(const float* A, int d, int d_out, _Float16* W, hipStream_t st);
hipError_t launch_rotate_f16(const _Float16* W, int d, int d_out, const _Float16* P, int64_t n, _Float16* Y, hipStream_t st);
hipError_t launch_rot_queries(const float* A, int d, int d_out, const float* q, int nq, float* out, hipStream_t st);
hipError_t launch_rot_back(const float* A, int d, int d_out, const float* dec, int64_t n, float* out, hipStream_t st);
hipError_t launch_xty(const _Float16* X, const float* Y, int64_t n, int d, float* G, hipStream_t st);
hipError_t launch_pq_scatter_codes(const uint8_t* src, int64_t n, int M, const int32_t* lists, const int32_t* pos, const int64_t* ids,
                                   const unsigned* tile0, int64_t id_lo, int64_t n_ids, uint8_t* codes, int64_t* idmap, uint32_t* inv,
                                   hipStream_t st);

// ---- IVF-SQ8 (knn_sq_kernels.hip): faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit), inner product, not residual.
// One code byte per column in the list-sorted, tile-padded arena; vmin / scale / step: device f32 [d] (include/knnx.h: "IVF-SQ8").
constexpr int SQ_BURST = 8;  // dwordx4 loads a lane of the list scan keeps in flight per burst (256 columns)
// u [nq][d] = q * step scaled by a power of two per query, in the scan's column order (input of launch_prep_blocks); bq [nq] = <q, vmin
// + step / 2>; inv [nq] = the inverse of the power
hipError_t launch_sq_prep(const float* q_dev, int nq, int d, const float* vmin, const float* step, float* u, float* bq, float* inv,
                          hipStream_t st);
// the list scan of one multi-block pass: the IVF mode-0 fields of ScanArgs with the code arena in place of the rows
struct SqScanArgs {
  const uint8_t* codes;
  int d;
  const _Float16* qfrag;  // [nblk][d * 64] fragment images of u
  const float* bq;        // [32 nblk]
  const float* inv;       // [32 nblk]
  int nq, k, cap, grid;
  int* thr_g;
  float* part_s;
  uint32_t* part_i;
  int* part_n;
  const uint4* work;
  const unsigned* nwork;
  int nblk;
  unsigned work_stride;
  // threshold mode (launch_sq_range_scan; k, cap, thr_g and part_* are not read there)
  const float* rthr;      // [32 nblk] thresholds, strict; +INFINITY: the query is finished
  unsigned* rcnt;         // [32 nblk] hits per query, exact even past rcap
  unsigned rcap;          // hits a query's slice holds
  float* hit_s;           // [nq][rcap] scores
  uint32_t* hit_i;        // [nq][rcap] arena rows
};
hipError_t launch_sq_scan(const SqScanArgs& a, hipStream_t st);
// Threshold mode of the list scan: every valid row of the work lists whose score is > rthr[q] is appended to query q's slice as (score,
// arena row); rcnt is cleared first.  The scores are those of launch_sq_scan, bit for bit.
hipError_t launch_sq_range_scan(const SqScanArgs& a, hipStream_t st);
// out [nq] = rows in the lists whose mask (masks [ceil(nq / 32)][nlist], bit q % 32) names query q
hipError_t launch_sq_probed_rows(const unsigned* masks, const unsigned* size, int nlist, int nq, unsigned long long* out, hipStream_t st);
// encode n fp16 rows into their arena slots (tile0 == null: slot = i; idmap == null: codes only), laying down idmap / inv like launch_ivf_scatter
hipError_t launch_sq_encode(const _Float16* src, int64_t n, int d, const int32_t* lists, const int32_t* pos, const int64_t* ids,
                            int64_t id0, const unsigned* tile0, int64_t id_lo, int64_t n_ids, const float* vmin, const float* scale,
                            uint8_t* codes, int64_t* idmap, uint32_t* inv, hipStream_t st);
// out [n][d] = the decoded rows of n ids through inv; an id outside the index (-1) -> 0xFF bytes
hipError_t launch_sq_decode(const uint8_t* codes, int d, const float* vmin, const float* step, int64_t id_lo, int64_t n_ids,
                            const uint32_t* inv, const int64_t* ids, int64_t n, float* out, hipStream_t st);
// per-column min / max of n fp16 rows (d <= 1024) -> vmin_dev / vmax_dev f32 [d]; enc: 2 d ints of device scratch
hipError_t launch_sq_colminmax(const _Float16* X, int64_t n, int d, int* enc, float* vmin_dev, float* vmax_dev, hipStream_t st);

// ---- post filter of one request on the device (knn_filter_kernels.hip; the shared arithmetic: knnx_filter_plan.h) ----
// R f32 [n][d] -> unit rows in place over the columns [0, d_user) (one fmaf chain per row, a zero row stays zero); columns [d_user, d) <- 0.
// d % 4 == 0, d <= 4096
hipError_t launch_filter_normalise(float* R, int n, int d, int d_user, hipStream_t st);
// every pair i < j < n of the unit rows E with e_i . e_j > thr (exact f32, columns ascending) -> links (i << 16 | j) in no particular
// order; counters[FILTER_C_LINKS] (cleared by the caller) counts them all, only the first `cap` are kept.  n <= FILTER_MAX_K
hipError_t launch_filter_links(const float* E, int n, int d, int d_user, float thr, uint32_t* links, int cap, int* counters, hipStream_t st);
// drop[i] = KNNX_DROP_VIOLENT if the first maximum of vs[i][0..P) is entry 1 | KNNX_DROP_UNSAFE if ss[i][0] > sthr, for i < n;
// drop[n..k) = 0.  vs / ss may be null (no such filter)
hipError_t launch_filter_bits(const float* vs, int P, const float* ss, int S, float sthr, int n, int k, uint8_t* drop, hipStream_t st);
// drop[i] |= KNNX_DROP_DUPLICATE for every i < n that is not the smallest member of its component under the kept links; does nothing
// when counters[FILTER_C_LINKS] is 0 or above cap.  Writes counters[FILTER_C_ROUNDS] and counters[FILTER_C_BOUND].  One workgroup.
hipError_t launch_filter_cc(const uint32_t* links, int cap, int* counters, int n, uint8_t* drop, hipStream_t st);

}  // namespace knnx
