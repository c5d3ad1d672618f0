/*
 * knnx.h -- C ABI of the MI355X-native inner-product kNN (search half of the hot path).
 *
 * This is the boundary a clip-retrieval maintainer binds (ctypes stub in INTEGRATION.md)
 * to replace the faiss `Index` object held in `ClipResource.image_index/.text_index`
 * (reference clip_retrieval/clip_back.py:781-782, built by `load_index` :589-596).
 * Each entry point names the reference call it stands in for.  Plain pointers and
 * sizes only; no torch / faiss types.  All functions return 0 on success or a negative
 * KNNX_E_* code; knnx_last_error() gives a thread-local message.  Nothing throws.
 *
 * Index rows are stored as fp16 [ntotal, d] row-major, resident in HBM.  Scores are
 * the fp32 inner product of the fp16 row with the fp32 query (query split hi/lo into
 * two fp16 MFMA operands, fp32 accumulate).  Result order: score descending, ties by
 * ascending id; missing results are id -1 / score -FLT_MAX (faiss IP padding).
 */
#ifndef KNNX_H
#define KNNX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct knnx_index knnx_index;

enum {
  KNNX_OK = 0,
  KNNX_E_ARG = -1,        /* bad argument (null, d unsupported, k out of range ...) */
  KNNX_E_HIP = -2,        /* a HIP runtime call failed (message has the hipError) */
  KNNX_E_NOMEM = -3,      /* device allocation failed / capacity exceeded */
  KNNX_E_STATE = -4,      /* call not valid in this state (e.g. add on an attached index) */
  KNNX_E_UNSUPPORTED = -5 /* valid request this build has no kernel for */
};

#define KNNX_METRIC_INNER_PRODUCT 0 /* faiss.METRIC_INNER_PRODUCT; the only metric clip_back uses */
#define KNNX_MAX_K_FAST 64          /* k <= 64: single-scan LDS candidate queues               */
#define KNNX_MAX_K 131072           /* 64 < k <= 131072: one range scan above a sampled / extrapolated threshold, hits ranked on the
                                     * host (the reference advertises K = 100 000: README.md:301, clip_back.py:358)        */

/* faiss.IndexFlatIP(d) / faiss.read_index(...) (clip_back.py:589-596).  `device` is the HIP
 * ordinal.  d must be a multiple of 256 and <= 1024 (CLIP embedding widths 512/768/1024). */
int knnx_create(int device, int d, int metric, knnx_index** out);
void knnx_destroy(knnx_index* ix);

/* Pre-size the HBM arena for n_rows rows (one hipMalloc; 288 GB parts leave no room to
 * grow by doubling).  Optional: add() grows geometrically if it was not called. */
int knnx_reserve(knnx_index* ix, int64_t n_rows);

/* faiss Index.add(x): append n rows.  Host pointers (pageable ok).  _f16 takes the exact
 * bytes of an `img_emb_*.npy` payload (clip_inference/writer.py:67-75); _f32 rounds to fp16
 * on the device. ids are implicit: id_base + row ordinal. */
int knnx_add_f16(knnx_index* ix, const uint16_t* rows, int64_t n);
int knnx_add_f32(knnx_index* ix, const float* rows, int64_t n);

/* Borrow n rows of fp16 already resident in HBM (caller keeps ownership; used by the
 * benchmark's on-device generator and by shard loaders that hipMemcpy themselves). */
int knnx_attach_device_f16(knnx_index* ix, const void* dev_rows, int64_t n);

/* faiss Index.reset(): drop all rows, keep the arena (flat indexes; the per-request dedup index of clip_back.py:290-294). */
int knnx_reset(knnx_index* ix);

/* Global id of local row 0 (row-sharded multi-GPU index: shard g has id_base = g*N/G). */
int knnx_set_id_base(knnx_index* ix, int64_t id_base);

/* faiss Index.ntotal / Index.d (ivf_metadata_ordering.py:51). */
int64_t knnx_ntotal(const knnx_index* ix);
int knnx_dim(const knnx_index* ix);

/* faiss Index.search(x, k) (clip_filter.py:55) and Index.search_and_reconstruct(x, k)
 * (clip_back.py:362).  q: host f32 [n, d] C-contiguous.  D: f32 [n, k], I: int64 [n, k],
 * R (may be NULL): f32 [n, k, d] (rows of id -1 are filled with 0xFF bytes like faiss).
 * Re-entrant; concurrent callers are serialised on the index's stream.  One pass over HBM serves up to 32 queries
 * (exact hi/lo scores), 64 (wide scan + proof) or, on flat indexes of >= 2 Mi rows with k <= 48, 256 queries (128 at
 * d = 1024): the register-stationary scan of csrc/knn_rq_kernels.hip; every path returns the exact top-k. */
int knnx_search(knnx_index* ix, const float* q, int n, int k, float* D, int64_t* I, float* R);

/* Same with every buffer already in HBM (benchmark / all-gather path).  `stream` is a
 * hipStream_t (NULL = the index's own stream).  Asynchronous on that stream; k <= 64.  The handle's scratch is shared
 * by all calls: consecutive calls are ordered by an event even when they use different streams. */
int knnx_search_device(knnx_index* ix, const float* q_dev, int n, int k, float* D_dev,
                       int64_t* I_dev, void* stream);

/* faiss Index.reconstruct_batch: ids are global; out f32 [n, d]; id -1 -> 0xFF fill. */
int knnx_reconstruct(knnx_index* ix, const int64_t* ids, int64_t n, float* out);

/* faiss Index.range_search(x, thresh) (clip_filter.py:52; clip_back.py:294 on k<=3000 rows):
 * all rows with <q,x> > thresh.  Two calls: pass I=D=NULL to get lims[n+1] (prefix counts),
 * then call again with buffers of lims[n] entries.  Ids ascending inside each query. */
int knnx_range_search(knnx_index* ix, const float* q, int n, float thresh, int64_t* lims,
                      float* D, int64_t* I);
/* The same in ONE pass for a caller with a good guess of the result size (the per-request dedup, clip_back.py:290-294):
 * lims [n + 1] is always filled; if lims[n] <= capacity the hits are written to D / I and the call returns 0, otherwise
 * D / I are left alone and it returns 1 (retry with knnx_range_search and lims[n] entries). */
int knnx_range_search_once(knnx_index* ix, const float* q, int n, float thresh, int64_t* lims, float* D, int64_t* I,
                           int64_t capacity);

/* faiss IndexIVFFlat(quantizer=IndexFlatIP, d, nlist, METRIC_INNER_PRODUCT) (the index family of BASELINE config 5;
 * the reference gets its indices from autofaiss, clip_index.py:12-66).  Protocol: knnx_add_* the rows GROUPED BY LIST
 * (list 0 first), then call knnx_ivf_set_lists once: centroids fp16 [nlist, d] (the coarse quantiser is a flat scan
 * over them), list_sizes [nlist], ids [ntotal] = the id each added row carries (a permutation of
 * [id_base, id_base + ntotal)).  Afterwards knnx_search* probe the nprobe lists whose centroids score highest for the
 * query (faiss `nprobe`, clip_back.py:357-369) and return exactly the top-k of those lists' rows (k up to KNNX_MAX_K;
 * fewer rows than k in the probed lists: -1 / -FLT_MAX padding like faiss); knnx_range_search returns the rows of the probed
 * lists above the threshold (faiss IndexIVF.range_search; clip_filter.py:52).  add is refused on an IVF index. */
int knnx_ivf_set_lists(knnx_index* ix, int nlist, const uint16_t* centroids_f16, const int64_t* list_sizes,
                       const int64_t* ids);
int knnx_ivf_set_nprobe(knnx_index* ix, int nprobe); /* 1 .. nlist (BASELINE config 5: 16 / 64 / 256) */
int knnx_ivf_nlist(const knnx_index* ix);
int knnx_ivf_nprobe(const knnx_index* ix);  /* the value knnx_ivf_set_nprobe left (1 after knnx_ivf_set_lists / knnx_ivf_end) */

/* ---- IVF-Flat build on the device (stands in for the autofaiss call of clip_index.py:12-66) ----------
 * Training: a builder keeps the centroids and a training sample resident in HBM.  One Lloyd iteration =
 * knnx_ivfb_assign_sample (argmax over the centroids by the MFMA assignment kernel; ties -> smaller list id) + host
 * bookkeeping (stable sort of the list ids -> order, prefix sums -> off) + knnx_ivfb_update (unit-norm mean of each list's members -- spherical k-means, what inner-product assignment needs --,
 * fixed summation order; empty lists keep their centroid for the caller to re-seed through knnx_ivfb_set_centroids).
 * Adding without a second copy of the shard: pass 1 knnx_ivfb_assign streams the rows and returns their list ids;
 * pass 2 knnx_ivf_begin(list sizes) / knnx_ivf_add_assigned(rows, ids, list, position inside the list) / knnx_ivf_end
 * scatters the rows straight into the list-sorted, tile-padded arena of an empty index.  Host pointers throughout. */
typedef struct knnx_ivf_builder knnx_ivf_builder;
int knnx_ivfb_create(int device, int d, int nlist, knnx_ivf_builder** out);
void knnx_ivfb_destroy(knnx_ivf_builder* b);
int knnx_ivfb_set_centroids(knnx_ivf_builder* b, const uint16_t* centroids_f16);
int knnx_ivfb_get_centroids(knnx_ivf_builder* b, uint16_t* centroids_f16);
int knnx_ivfb_set_sample(knnx_ivf_builder* b, const uint16_t* rows_f16, int64_t n);
int knnx_ivfb_assign_sample(knnx_ivf_builder* b, int32_t* lists_out);
int knnx_ivfb_update(knnx_ivf_builder* b, const int64_t* order, const int64_t* off);
int knnx_ivfb_assign(knnx_ivf_builder* b, const uint16_t* rows_f16, int64_t n, int32_t* lists_out);
int knnx_ivf_begin(knnx_index* ix, int nlist, const uint16_t* centroids_f16, const int64_t* list_sizes);
int knnx_ivf_add_assigned(knnx_index* ix, const uint16_t* rows_f16, int64_t n, const int64_t* ids, const int32_t* lists,
                          const int32_t* pos);
int knnx_ivf_end(knnx_index* ix);
/* The same build for rows that are ALREADY IN HBM (BASELINE config 5: a 125 M x 1024 shard is 256 GB of the 288 GB -- it is
 * produced on the GPU and can neither visit host memory nor exist twice).  Device pointers; every call is synchronous.
 *   training   knnx_ivfb_set_sample_device (borrows the caller's sample rows), knnx_ivfb_seed_from_sample (initial centroids and
 *              re-seeding of empty lists: centroid list_ids[i] := sample row sample_rows[i]; host index arrays),
 *              knnx_ivfb_lloyd = one whole iteration (assign, counting sort on the host, update); sizes_out [nlist] or NULL
 *   pass 1     knnx_ivfb_assign_device: lists_dev[i] = list of row i, list sizes accumulate in the builder ->
 *              knnx_ivfb_list_sizes (host int64 [nlist]; reset != 0 clears the counters)
 *   pass 2     knnx_ivf_begin(sizes) ... knnx_ivf_add_assigned_device (row i carries id id0 + i and takes the next free
 *              position of its list) ... knnx_ivf_end
 * knnx_ivf_add_assigned (host) and _device both refuse a list id out of range, a position outside its list and a (list,
 * position) used twice; knnx_ivf_end refuses a list that did not receive its announced number of rows. */
int knnx_ivfb_set_sample_device(knnx_ivf_builder* b, const void* rows_dev_f16, int64_t n);
int knnx_ivfb_seed_from_sample(knnx_ivf_builder* b, const int32_t* list_ids, const int64_t* sample_rows, int64_t n);
int knnx_ivfb_lloyd(knnx_ivf_builder* b, int64_t* sizes_out);
int knnx_ivfb_assign_device(knnx_ivf_builder* b, const void* rows_dev_f16, int64_t n, int32_t* lists_dev);
int knnx_ivfb_list_sizes(knnx_ivf_builder* b, int64_t* sizes_out, int reset);
int knnx_ivf_add_assigned_device(knnx_index* ix, const void* rows_dev_f16, int64_t n, int64_t id0, const int32_t* lists_dev);

/* ---- IVF-PQ: faiss IndexIVFPQ(IndexFlatIP(d), d, nlist, M, 8), METRIC_INNER_PRODUCT, by_residual = true ----------------------
 * (the index type autofaiss builds for large corpora -- clip_index.py:12-66; the reference notebook's OPQ256_768,IVF16384_HNSW32,PQ256x8
 * without the HNSW coarse quantiser; the OPQ rotation is the block below).  M in {16, 32, 64, 128} dividing d, or M = 256 with d in
 * {512, 768, 1024} (d / M = 2, 3, 4; PQ256x8); 256 centroids per sub-quantiser; other M, and M = 256 at d = 256:
 * KNNX_E_ARG.  Codebooks: f32 [M][256][d / M].  Row x of list l: residual r = f32(x_f16) - f32(c_l), code byte m =
 * argmin_j ||r_m - C[m][j]||^2 in fp32 (ties -> smaller j).  Score = <q, c_l> + sum over m (in order) of LUT[m][code_m], LUT[m][j] =
 * <q_m, C[m][j]> in fp32; the coarse quantiser and its probe rule are those of IVF-Flat.  Results as knnx_search; reconstruct /
 * the R of search returns the decoded vector f32(c_l) + concat_m C[m][code_m].
 * Build: knnx_ivfpq_set_quantizer on an empty index, then knnx_ivf_begin / knnx_ivf_add_assigned[_device] / knnx_ivf_end ENCODE
 * the rows (same list / position rules), or knnx_ivfpq_add_codes loads precomputed codes in their place.  The arena holds M bytes
 * per row (M + 12 with the id maps: 268 at M = 256 against 2 d + 12 for fp16 rows).
 * M = 256: the query's lookup table (256 KiB) does not fit the LDS, so the ADC stage runs in two halves of m: a first kernel stores,
 * for every row of the probed lists, the fp32 sum over m = 0 .. 127; the scan proper starts from that stored value and continues over
 * m = 128 .. 255.  A 4-byte store and load is exact, so the score is still cs + (ONE fp32 sum over m = 0 .. 255 in ascending order
 * from 0.f), and everything defined on the scores -- k <= 64, the refine store, the threshold scan, the rotation, the other entry
 * points -- holds at M = 256 word for word.  Memory rule: the partial sums take g x S x 4 bytes of scratch, S = the sum of the nprobe
 * largest list sizes of the index, g = the queries scored at once (<= 256); when 256 x S x 4 exceeds KNNX_PQ_PARTIAL_MAX_BYTES (read
 * from the environment by knnx_ivfpq_set_quantizer; default 1 GiB, a guess nobody has measured) a pass scores its queries in consecutive
 * sub-groups of g = max(1, budget / (S x 4)); results do not depend on g.  A buffer that cannot be had: KNNX_E_NOMEM naming the bytes.
 * An index with M <= 128 allocates and launches nothing of this.  k > 64 and range_search answer KNNX_E_UNSUPPORTED (unless switched on: knnx_ivfpq_set_threshold_scan below); add / attach / synth_fill / reset / reserve / knnx_ivf_set_lists
 * answer KNNX_E_STATE.  At most 2^32 - 1 padded rows per device. */
int knnx_ivfpq_set_quantizer(knnx_index* ix, int M, const float* codebooks);
int knnx_ivfpq_add_codes(knnx_index* ix, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists, const int32_t* pos);
int knnx_ivfpq_m(const knnx_index* ix); /* 0: not an IVF-PQ index */
/* every row of a built index, in arena order (list by list): ids [ntotal], lists [ntotal], codes [ntotal][M] (host) */
int knnx_ivfpq_get_codes(knnx_index* ix, int64_t* ids, int32_t* lists, uint8_t* codes);
int knnx_ivfpq_get_codebooks(knnx_index* ix, float* codebooks);
/* ---- OPQ rotation in front of IVF-PQ: faiss IndexPreTransform(OPQMatrix(d, M), IndexIVFPQ(...)), d_out = d_in = d (d_out > d_in: below)
 * (what autofaiss puts in front of every IVF-PQ index it builds, and what ivf_metadata_ordering.py:23-24 applies to a query before it
 * asks the coarse quantiser).  A: f32 [d][d] row-major, y = A x, owned by the index.  Everything of the block above -- centroids, lists,
 * residuals, codebooks, codes, LUT, the ADC scan -- lives in the rotated space; an index without a rotation is exactly that block.
 *   rows      a row entering the build is x_f16; what is encoded is y = fp16(A f32(x_f16)): A = hi + lo / 2048 with hi = fp16(A), lo =
 *             fp16(2048 (A - hi)); per component one fp32 accumulator takes the lo products, 32 columns per MFMA step in ascending
 *             order, is scaled by 2^-11, takes the hi products in the same order and is rounded to fp16 once (a zero sum is +0).  From
 *             there on y is "the row" of the definition above.  The list ids handed to knnx_ivf_add_assigned[_device] are those of the
 *             ROTATED rows (knnx_rotate_f16_device, then the assignment); the rows handed over are UN-ROTATED, the index rotates each
 *             chunk itself before it encodes.  knnx_ivfpq_add_codes is unchanged: codes are already in the rotated space.
 *   queries   q' = A q in fp32, once per query at the head of the pass: lane l of 64 sums columns l, l + 64, ... in ascending order with
 *             fmaf, the 64 partial sums are added pairwise (a butterfly over lane distance 32, 16, .. 1).  Coarse scores, probe set
 *             and LUT come from q'.  A is orthonormal, so the scores still estimate <q, x>.
 *   decoding  reconstruct, the R of search / search_dedup and the vectors the dedup links are computed from are in the ORIGINAL space:
 *             A^T (f32(c_l) + concat_m C[m][code_m]), fp32, component c = sum over j ascending of A[j][c] * decoded[j] with fmaf
 *             (faiss IndexPreTransform::reconstruct -> reverse_transform; clip_back.py:290-325, 362-378 expects un-rotated rows).
 * knnx_ivfpq_set_rotation: on an IVF-PQ index after knnx_ivfpq_set_quantizer and before knnx_ivf_begin, KNNX_E_STATE otherwise and on
 * any index that is not IVF-PQ; a matrix with max |A A^T - I| > 1e-3 is refused (KNNX_E_ARG): scores of another metric would be silent.
 * knnx_ivfpq_get_rotation: 0 and the matrix, or 1 and A untouched when the index has none.  knnx_shards_adopt takes IVF-PQ shards that
 * all carry the same rotation (bit for bit) or none, and refuses a mix. */
int knnx_ivfpq_set_rotation(knnx_index* ix, const float* A);
int knnx_ivfpq_get_rotation(knnx_index* ix, float* A);
/* ---- d_out > d_in: faiss IndexPreTransform(OPQMatrix(d_in, M, d_out), IndexIVFPQ(..., d_out, ...)) ("OPQ256_768,...,PQ256x8" on 512-d rows) --
 * The index has two widths.  d (= d_in, knnx_dim) is what the user sees: queries, the rows entering the build, the refine store and its
 * re-scoring, knnx_reconstruct, the R of search / search_dedup and the dedup vectors.  d_out is the quantiser space: centroids fp16
 * [nlist][d_out], the coarse scan, residuals, codebooks f32 [M][256][d_out / M], LUT, codes, the decode scratch.  A: f32 [d_out][d]
 * row-major with orthonormal COLUMNS (A^T A = I_d), y = A x; <A q, A x> = <q, x>, so the scores still estimate the inner product; the back
 * transform is A^T y.  The arithmetic contracts of the OPQ block above (rows / queries / decoding) hold word for word with "columns"
 * meaning the d columns of A: a row's component j sums the d columns of row j of A, a query's likewise, and decoding sums j over the
 * d_out rows of A.  Supported: both widths multiples of 256, 256 <= d < d_out <= 1024.  An index nobody gave a d_out is exactly the
 * blocks above and below, byte for byte.
 * knnx_ivfpq_set_out_dim: on an empty index BEFORE knnx_ivfpq_set_quantizer; KNNX_E_STATE afterwards or on an index that has rows or
 * lists; KNNX_E_ARG for a width outside the rule (the message names both widths); d_out == d is accepted and changes nothing.
 * knnx_ivfpq_out_dim: d_out, or d when none was set; 0 on a null or non-PQ index.  With a d_out != d:
 *   quantizer  knnx_ivfpq_set_quantizer applies its M rule to d_out and takes codebooks [M][256][d_out / M] (knnx_ivfpq_get_codebooks too).
 *   rotation   knnx_ivfpq_set_rotation / knnx_ivfpq_get_rotation take and give [d_out][d]; refused (KNNX_E_ARG) unless
 *              max |A^T A - I_d| <= 1e-3 in float64 (a square matrix keeps the A A^T test above).  The rotation is MANDATORY:
 *              knnx_ivf_begin without one answers KNNX_E_STATE and says why.
 *   build      knnx_ivf_begin takes centroids fp16 [nlist][d_out]; knnx_ivf_add_assigned[_device] take UN-ROTATED rows [n][d], the
 *              list ids being those of the rotated rows as above; knnx_ivfpq_add_codes is unchanged.
 *   refine     the row arena is tiles x 32 x d x 2 bytes (memory rule: M + 2 d_in bytes per padded row), which is what
 *              knnx_ivfpq_arena_bytes reports; re-scoring uses the original d-wide query.
 *   shards     knnx_shards_adopt takes shards with the same d_out and the same rotation bit for bit and refuses a mix (the message names
 *              the widths); queries travel to the shards d wide. */
int knnx_ivfpq_set_out_dim(knnx_index* ix, int d_out);
int knnx_ivfpq_out_dim(const knnx_index* ix); /* d when no d_out was set; 0: null or not an IVF-PQ index */
/* ---- Refine store on IVF-PQ: faiss IndexRefineFlat(IndexIVFPQ(...)) ("...,PQ64,RFlat"), with or without the OPQ rotation ------------
 * The index keeps, next to the codes, the fp16 rows exactly as they entered the build (original, UN-ROTATED space), in the
 * list-sorted, tile-padded arena order of the codes: tiles x 32 x d x 2 bytes more HBM (memory rule: M + 2 d bytes per padded row;
 * the id map and its inverse serve codes and rows alike).
 *   search    k <= 64, kc = k x k_factor.  1. Candidates: the top kc rows of the probed lists by (ADC score descending, id ascending) --
 *             what knnx_search would return for k = kc; coarse quantiser, probe rule, LUT and summation order are those of the block
 *             above; all rows of the probed lists when they hold fewer than kc.  2. Re-score: s = <f32(x_f16), q> in fp32 with the
 *             ORIGINAL query and the stored row (with a rotation q' = A q feeds the candidate stage only).  Summation order: lane l of
 *             64 owns columns 8 (64 p + l) .. 8 (64 p + l) + 7 for p = 0, 1 (while below d) and runs ONE fmaf chain from 0 over them in
 *             ascending order; the 64 lane sums are added pairwise in a butterfly over lane distance 32, 16, .. 1.  It depends on
 *             nothing else: a query gets the same D bits alone, in a batch of 256 and through the coalescer.  3. Result: the top k of
 *             the candidates by (exact score descending, id ascending), padded with -1 / -FLT_MAX.
 *   rows      reconstruct, the R of search / search_dedup and the vectors the dedup links are computed from are the STORED rows,
 *             f32(x_f16) bit for bit: no decode, no back-rotation (faiss IndexRefine::reconstruct).
 * knnx_ivfpq_set_refine: after knnx_ivfpq_set_quantizer and before knnx_ivf_begin (either order with knnx_ivfpq_set_rotation);
 * KNNX_E_STATE otherwise and on any index that is not IVF-PQ.  knnx_ivf_begin then allocates the row arena next to the code arena
 * (after giving back what an index gives back for its own data; KNNX_E_NOMEM leaves the index empty), knnx_ivf_add_assigned[_device]
 * store the un-rotated chunk AND encode it; knnx_ivfpq_add_codes answers KNNX_E_STATE (it has no rows to store).
 * knnx_ivfpq_set_k_factor: 1 .. 512, default 1 (faiss' default: the plain index's ids with exact scores); any time, any IVF-PQ index
 * (without a refine store it has no effect).  A search with k x k_factor > 512 answers KNNX_E_ARG and names both numbers.  k > 64 and
 * range_search stay KNNX_E_UNSUPPORTED unless the threshold scan is switched on (next block).  knnx_shards_adopt takes IVF-PQ shards that all have a refine store or all have none and refuses
 * a mix; each shard refines its own candidates and the merge ranks the exact scores.  An index without a refine store is exactly the
 * two blocks above.  knnx_ivfpq_arena_bytes: bytes of the code arena and of the row arena (0 without a refine store). */
int knnx_ivfpq_set_refine(knnx_index* ix, int on);
int knnx_ivfpq_refine(const knnx_index* ix); /* 1: the index has (or will be built with) a refine store */
int knnx_ivfpq_set_k_factor(knnx_index* ix, int k_factor);
int knnx_ivfpq_k_factor(const knnx_index* ix);
int knnx_ivfpq_arena_bytes(knnx_index* ix, int64_t* code_bytes, int64_t* row_bytes);
/* ---- Threshold scan on IVF-PQ: k > 64 and range_search (clip_back.py:356-369 asks for up to 1e5 results; clip_filter.py:52) ---------
 * A switch per index, OFF by default: an index nobody switched on is exactly the three blocks above, refusals included.
 * knnx_ivfpq_set_threshold_scan: any IVF-PQ index, any time (like knnx_ivfpq_set_k_factor); KNNX_E_STATE on an index that is not IVF-PQ.
 * knnx_ivfpq_threshold_scan: 0 / 1; 0 on a non-PQ or null index.  With the switch ON:
 *   search    64 < k <= 131072: the top k rows of the probed lists by (ADC score descending, id ascending), padded with -1 / -FLT_MAX
 *             -- the contract of the IVF-PQ block for k <= 64, extended.  The scores are the SAME fp32 values (same LUT, cs + (sum over m
 *             in order)), so the first 64 results of a k > 64 search equal the k = 64 search bit for bit, D and I, and a query gets the
 *             same answer alone and in a batch.  R comes from knnx_reconstruct: decoded and back-rotated rows, or the stored rows of a
 *             refine store.  How: the ADC scan in threshold mode (every row scoring > t is a hit) with t walked down from the query's
 *             64th score until at least k rows pass; the hits are ranked on the host.
 *   range     knnx_range_search / knnx_range_search_once on an index WITHOUT a refine store: all rows of the probed lists whose ADC score
 *             is > thresh (strict), ids ascending inside each query; two-call protocol, _once contract and KNNX_E_STATE on mismatching
 *             lims as for IVF-Flat.  Behind a rotation the scores are those of q' = A q.  On an index WITH a refine store it stays
 *             KNNX_E_UNSUPPORTED (the message says "refine store"): it would need the exact score of every probed row.
 *   refine    k > 64: kc = k x k_factor candidates by (ADC score, id) as above, re-scored as the refine block defines (same summation
 *             order), the top k by (exact score descending, id ascending) returned.  kc > 131072 answers KNNX_E_ARG and names both
 *             numbers.  k <= 64 keeps the refine block's path and its k x k_factor <= 512 rule.
 * knnx_search_device, knnx_search_dedup and the coalescer stay at k <= 64; builds and knnx_ivfpq_add_codes are unchanged.  Shards: every
 * shard answers for itself (a shard with the switch off gives its own refusal).  knnx_ivfpq_threshold_stats: counters since the index
 * was created -- queries served with k > 64, threshold-scan launches (one serves a whole group of queries), scans summed over the
 * queries that took part in them, hits fetched to the host; any pointer may be null. */
int knnx_ivfpq_set_threshold_scan(knnx_index* ix, int on);
int knnx_ivfpq_threshold_scan(const knnx_index* ix);   /* 0 / 1; 0 on a non-PQ or null index */
int knnx_ivfpq_threshold_stats(knnx_index* ix, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits);
/* The row rotation on its own (the MFMA kernel of the build): out_dev[i] = fp16(A rows_dev[i]) as defined above, n fp16 rows in HBM,
 * d in {256, 512, 768, 1024}; A_host f32 [d][d] is NOT checked for orthonormality; out_dev must not overlap rows_dev; rows past n are
 * not written.  knnx_xty_device: G = X^T Y (device f32 [d][d]) for fp16 rows X and f32 rows Y [n][d] in HBM, every element one fp32
 * fmaf chain over the rows in ascending order -- the product whose SVD is the Procrustes step of OPQ training.  `stream`: hipStream_t
 * or NULL; both synchronous. */
int knnx_rotate_f16_device(int device, const float* A_host, const void* rows_dev_f16, int64_t n, int d, void* out_dev_f16, void* stream);
/* The same for A_host f32 [d_out][d_in], d_in <= d_out, both in {256, 512, 768, 1024}: rows_dev fp16 [n][d_in], out_dev fp16 [n][d_out]. */
int knnx_rotate_rect_f16_device(int device, const float* A_host, const void* rows_dev_f16, int64_t n, int d_in, int d_out,
                                void* out_dev_f16, void* stream);
int knnx_xty_device(int device, const void* x_dev_f16, const float* y_dev_f32, int64_t n, int d, float* g_dev, void* stream);
/* Codebook training on the device (faiss trains the M sub-quantisers on the residuals of a sample; default 256 x 256 rows):
 * the builder keeps the sample rows (fp16 [n][d]) with their list ids and the coarse centroids resident.  knnx_pqb_lloyd = one
 * iteration of all M L2 k-means: assignment (the encode kernel), counting sort on the host, fixed-order mean update; an empty
 * cluster keeps its codeword (codes_out [n][M], sizes_out [M][256] or NULL).  knnx_pqb_seed_from_sample: entry mj[i] = m * 256 + j
 * := residual sub-vector m of sample row sample_rows[i] (initial codebooks, re-seeding).  _set_sample_device borrows the rows. */
typedef struct knnx_pq_builder knnx_pq_builder;
int knnx_pqb_create(int device, int d, int M, knnx_pq_builder** out);
void knnx_pqb_destroy(knnx_pq_builder* b);
int knnx_pqb_set_sample(knnx_pq_builder* b, const uint16_t* rows_f16, const int32_t* lists, int64_t n, const uint16_t* centroids_f16,
                        int nlist);
int knnx_pqb_set_sample_device(knnx_pq_builder* b, const void* rows_dev_f16, const int32_t* lists_dev, int64_t n,
                               const uint16_t* centroids_f16, int nlist);
int knnx_pqb_seed_from_sample(knnx_pq_builder* b, const int32_t* mj, const int64_t* sample_rows, int64_t n);
int knnx_pqb_set_codebooks(knnx_pq_builder* b, const float* codebooks);
int knnx_pqb_get_codebooks(knnx_pq_builder* b, float* codebooks);
int knnx_pqb_lloyd(knnx_pq_builder* b, uint8_t* codes_out, int64_t* sizes_out);

/* ---- IVF-SQ8: faiss IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, QT_8bit, METRIC_INNER_PRODUCT), by_residual = false -------------
 * (the "IVF65536,SQ8" factory string: the point between IVF-Flat's 2 d + 12 and IVF-PQ's M + 12 bytes per row).  The arena holds ONE
 * byte per dimension: d + 12 bytes per padded row with the id maps; pad rows of a tile are zero bytes and are never admitted.  The
 * quantiser is NOT residual: two fp32 vectors vmin [d], vdiff [d] (faiss' `trained` of QT_8bit).  The library derives, on the HOST in
 * fp32 with IEEE division (numpy float32 gives the same bits): scale_j = 255.f / vdiff_j, step_j = vdiff_j / 255.f, and scale_j = 0
 * where vdiff_j == 0 (a constant column; zero-padded columns are such).
 *   encode    t = (f32(x_f16_j) - vmin_j) * scale_j, ONE fp32 subtract then ONE fp32 multiply (no fused contraction); code_j = 0 if
 *             t < 0 or t is NaN, 255 if t >= 255, (int)t otherwise -- faiss' (int)(255 * x) on the clamped, normalised component;
 *             equal to np.clip(np.floor((x.astype(f32) - vmin) * scale), 0, 255) bit for bit.
 *   decode    dec_j = vmin_j + (f32(code_j) + 0.5f) * step_j, the multiply and the add rounded separately.  knnx_reconstruct, the R
 *             of search / search_dedup and the vectors the dedup links are computed from are these rows, bit-equal to the numpy
 *             float32 restatement.
 *   score     <q, dec(row)>, evaluated as b_q + sum_j u_j code_j with u = q * step and b_q = <q, vmin + step / 2>: the codes enter the
 *             MFMA as fp16 values (0 .. 255 are exact), u -- scaled by a power of two per query so that it sits in the fp16 normal
 *             range, which is undone exactly -- is split hi / lo into two fp16 operands as the fp16 scans split q, accumulation is
 *             fp32, b_q is added once per score.  Not a bit-level contract: within 1e-5 of the float64 value, like the fp16 and ADC
 *             scans.  A (query, row) score does not depend on the batch the query arrives in.
 *   the rest  coarse quantiser, probe rule (knnx_ivf_set_nprobe), result order (score descending, ties by ascending id) and the
 *             -1 / -FLT_MAX padding are IVF-Flat's, word for word.
 * Build: knnx_ivfsq_set_quantizer on an EMPTY index before knnx_ivf_begin (KNNX_E_ARG for a non-finite entry or a negative vdiff;
 * KNNX_E_STATE on an index that has rows or lists, that already has a quantiser, or that is IVF-PQ -- and knnx_ivfpq_set_quantizer
 * answers KNNX_E_STATE on an IVF-SQ8 index).  Afterwards knnx_ivf_begin / knnx_ivf_add_assigned[_device] / knnx_ivf_end ENCODE the
 * rows under the same list / position rules, or knnx_ivfsq_add_codes loads precomputed codes [n][d] in their place (the scatter
 * alone).  knnx_ivfsq_get_quantizer: vmin / vdiff as they were given.  knnx_ivfsq_get_codes: every row of a built index in arena
 * order (list by list): ids [ntotal], lists [ntotal], codes [ntotal][d] (host).  knnx_ivfsq: 1 on an IVF-SQ8 index, 0 otherwise.
 * Served: knnx_search (with and without R), knnx_search_device, knnx_search_dedup, the coalescer, knnx_reconstruct,
 * knnx_ivf_set_nprobe, knnx_ivf_id_order / knnx_ivf_map_ids, knnx_ivf_last_scan_tiles (bytes read = tiles * 32 * d), and
 * knnx_shards_adopt of IVF-SQ8 shards that carry the same quantiser bit for bit (a different one, or a mix with another index kind,
 * is refused with a message) -- all with k <= 64 and any n: every batch is ONE multi-block pass per 256 queries (1 .. 32 queries are
 * one block), so the ids do not depend on the batch size.  Refused: k > 64 and knnx_range_search* answer KNNX_E_UNSUPPORTED unless the
 * threshold scan is switched on (next block); add /
 * attach / synth_fill / reset / reserve / knnx_ivf_set_lists answer KNNX_E_STATE; every such message says "IVF-SQ8".  An index nobody
 * gave an SQ8 quantiser is exactly the blocks above and below, byte for byte: it allocates and launches nothing of this. */
int knnx_ivfsq_set_quantizer(knnx_index* ix, const float* vmin, const float* vdiff);
int knnx_ivfsq_get_quantizer(knnx_index* ix, float* vmin, float* vdiff);
int knnx_ivfsq(const knnx_index* ix); /* 0 / 1 */
int knnx_ivfsq_add_codes(knnx_index* ix, const uint8_t* codes, int64_t n, const int64_t* ids, const int32_t* lists, const int32_t* pos);
int knnx_ivfsq_get_codes(knnx_index* ix, int64_t* ids, int32_t* lists, uint8_t* codes);
/* ---- Threshold scan on IVF-SQ8: k > 64 and range_search (clip_back.py:356-369 asks for up to 1e5 results; clip_filter.py:52) --------
 * A switch per index, OFF by default: an index nobody switched on is exactly the block above, refusals included (the two messages
 * byte for byte), and allocates and launches nothing of this.
 * knnx_ivfsq_set_threshold_scan: any IVF-SQ8 index, any time; KNNX_E_STATE on any other index (the message says "IVF-SQ8").
 * knnx_ivfsq_threshold_scan: 0 / 1; 0 on a non-SQ8 or null index.  With the switch ON:
 *   search    64 < k <= 131072: the top k rows of the probed lists by (score descending, id ascending), padded with -1 / -FLT_MAX -- the
 *             contract of the IVF-SQ8 block for k <= 64, extended.  The scores are the SAME fp32 values (same operands, same MFMA order,
 *             same two roundings around inv_q and b_q), so the first 64 results of a k > 64 search equal the k = 64 search bit for bit,
 *             D and I, and a query gets the same ids alone and in a batch.  R comes from knnx_reconstruct: the decoded rows.  How: the
 *             code scan in threshold mode (every valid row of the probed lists scoring > t is a hit) with t walked down from the
 *             query's 64th score until at least k rows pass; queries run in groups of up to 256 over ONE coarse half and ONE set of work
 *             lists, one launch and one synchronisation per step; the hits are ranked on the host.
 *   range     knnx_range_search / knnx_range_search_once: all rows of the probed lists whose score is > thresh (strict), ids ascending
 *             inside each query; two-call protocol, the _once return value 1 and KNNX_E_STATE on mismatching lims as for IVF-Flat.
 * knnx_search_device, knnx_search_dedup and the coalescer stay at k <= 64 and keep their messages; builds and knnx_ivfsq_add_codes are
 * unchanged.  Shards: every shard answers for itself (a shard with the switch off gives its own refusal).
 * knnx_ivfsq_threshold_stats: counters since the index was created -- queries served with k > 64, threshold-scan launches (one serves
 * a whole group of queries), launches summed over the queries that took part in them, hits fetched to the host; any pointer may be null. */
int knnx_ivfsq_set_threshold_scan(knnx_index* ix, int on);
int knnx_ivfsq_threshold_scan(const knnx_index* ix);   /* 0 / 1; 0 on a non-SQ8 or null index */
int knnx_ivfsq_threshold_stats(knnx_index* ix, int64_t* queries, int64_t* launches, int64_t* query_scans, int64_t* hits);
/* The training kernel (faiss RS_minmax with argument 0): per-column min and max of n fp16 rows [n][d] in HBM, 0 < d <= 1024, n > 0 ->
 * host f32 vmin_out [d], vmax_out [d].  Min and max do not depend on the order of the rows: bit-equal to numpy's
 * x.astype(float32).min(0) / .max(0).  `stream`: hipStream_t or NULL; synchronous. */
int knnx_colminmax_device(int device, const void* rows_dev_f16, int64_t n, int d, float* vmin_out, float* vmax_out, void* stream);

/* ---- List-ordered ids: the reference's reorder_metadata_by_ivf_index (ivf_metadata_ordering.py:17-64, clip_back.py:350-369, 629-640) ----
 * A metadata store re-ordered so that the ids of one inverted list are one contiguous run turns the k random rows of a request into
 * nprobe runs.  The mapping is a function of the layout a built IVF index (IVF-Flat, IVF-SQ8 or IVF-PQ; with or without rotation, d_out, refine
 * store, threshold scan) already owns.  size[l] = rows of list l; dense0[l] = the exclusive prefix sum of size in int64.  The row at
 * position j of list l (arena row 32 * tile0[l] + j) has the ORDINAL dense0[l] + j; the ordinals are a permutation of [0, ntotal); pad
 * rows have none.
 *   new_to_old[o] = the id of the row with ordinal o: the lists' ids one after the other, list 0 first, in arena order (what faiss'
 *                   il.get_ids(l) yields list by list).
 *   old_to_new[i] = id_base + the ordinal of the row whose id is id_base + i, i in [0, ntotal).  With id_base = 0 exactly the array
 *                   get_old_to_new_mapping returns.
 * knnx_ivf_id_order: host arrays of ntotal int64 each; one may be NULL, both NULL: KNNX_E_ARG.  The export walks consecutive ranges of
 * KNNX_ID_ORDER_CHUNK ordinals (read from the environment at call time; default 2^22, minimum 64) through one staging buffer of that
 * size: no device allocation proportional to ntotal.
 * knnx_ivf_map_ids: out[i] = the old_to_new value of ids[i] (host, n entries); -1 -> -1; out may alias ids.  An id that is neither -1
 * nor in [id_base, id_base + ntotal) answers KNNX_E_ARG naming the id and its position; the range is checked on the host before
 * anything is launched and out is left untouched.  n == 0 is a success that launches nothing.  It is meant for the request path: it
 * does not take the lock the searches hold (the layout is immutable once the index is built) but a mutex, a stream and a grow-on-demand
 * staging of its own, walked in chunks of KNNX_ID_ORDER_CHUNK when n exceeds it; knnx_destroy waits for it.
 * Both answer KNNX_E_STATE, with a message that says why, on a flat index, on an IVF index between knnx_ivf_begin and knnx_ivf_end, and
 * on an empty index.  An index nobody asks for a mapping allocates and launches nothing of this: dense0 is built by the first call, from
 * the list sizes, and kept.  Nothing of it is saved with an index: it follows from the layout.
 * Shards: shard g holds the global ids [row_lo[g], row_hi[g)) with id_base = row_lo[g], so the global mapping is the concatenation of
 * the shards' mappings -- a permutation of [0, N), list-sorted inside each shard's range.  knnx_shards_map_ids routes every id to its
 * shard by row range, maps per shard and puts the answers back in request order; an id outside every range answers KNNX_E_ARG as above;
 * shards that are not IVF answer KNNX_E_STATE. */
int knnx_ivf_id_order(knnx_index* ix, int64_t* old_to_new, int64_t* new_to_old);
int knnx_ivf_map_ids(knnx_index* ix, const int64_t* ids, int64_t n, int64_t* out);

/* ---- Growing a built index: faiss index.add on a trained IVF index (autofaiss fills an index batch by batch) and merge_from / merge_ondisk
 * (clip_back_prepro/index_combiner.py joins index parts that share a quantiser) ----
 * For every BUILT IVF index -- IVF-Flat, IVF-PQ (rotation, d_out, refine store, M = 256, threshold scan) and IVF-SQ8; knnx_ivf_end or
 * knnx_ivf_set_lists has run -- that owns its rows.  knnx_add_* keeps refusing such an index; these are the calls that grow it.
 * Ids stay faiss' sequential ids: row i of a call gets id id_base + ntotal_before + i.  Inside its list a row goes behind the rows already
 * there, in call order -- position = old list size + its stable rank among the rows of the call in the same list.  The result is, bit for
 * bit (arena, id maps, search results, exported codes), the index knnx_ivf_begin / knnx_ivf_add_assigned / knnx_ivf_end build from the
 * concatenated rows with the same centroids, quantiser and lists.
 *   knnx_ivf_append_assigned  rows_f16 host fp16 [n][d]; lists host int32 [n] names the list of every row (in the quantiser space for an
 *                             index with a rotation, as at build time).
 *   knnx_ivf_append           the library assigns: the assignment kernel of knnx_ivfb_assign over the index's own coarse centroids, after
 *                             the rotation where the index has one.  lists_out (host int32 [n], may be NULL) receives the lists.
 *   knnx_ivf_append_device    the same for rows already in HBM on the index's device (fp16 [n][d]); the rows never visit the host.
 *   knnx_ivf_merge_from       every row of `other` into ix.  Both built and of the same kind; d, d_out, nlist, M equal; centroids,
 *                             codebooks, rotation and SQ8 ranges bit-equal; a refine store in both or in neither -- otherwise KNNX_E_ARG
 *                             naming what differs.  other's row with id j gets id id_base + ntotal_before + (j - other's id_base); inside
 *                             a list the rows keep other's order, behind the rows already there.  Codes and rows are copied, never
 *                             encoded again; they are staged through host memory (all of other at once), so the two may live on
 *                             different devices.  `other` is left UNTOUCHED (faiss' merge_from empties it).  ix == other: KNNX_E_ARG.
 * How: the arena is dense and tile-padded (tile0 = prefix sum of ceil(size / 32)), so a list that grows moves every list behind it.  A
 * call lays the grown index down OUT OF PLACE -- new arena(s), idmap and inv; the occupied tiles copied by a tile-granular move kernel,
 * the new rows scattered / encoded by the kernels of the build -- and swaps it in at the end: peak memory is old + new arena.  Calls are
 * all or nothing and atomic for searchers (they run under the lock the searches hold): a search from another thread sees the index
 * before or after the call.  Argument errors -- a NULL pointer, a list id outside [0, nlist), a flat index, an index between
 * knnx_ivf_begin and knnx_ivf_end, borrowed rows -- answer KNNX_E_ARG before anything is touched; an allocation that fails answers
 * KNNX_E_NOMEM, more than 2^32 padded rows KNNX_E_UNSUPPORTED; in every case nothing was added and the index stays searchable.
 * nprobe, k_factor, the refine and threshold-scan switches and the counters are kept.  The list-ordered ids (above) change with every
 * call -- every old_to_new entry may shift -- so a list-ordered metadata store must be exported again.  Per-list slack, in-place moves
 * and a sharded form are not provided; ids are removed by the block "Shrinking a built index" below. */
int knnx_ivf_append_assigned(knnx_index* ix, const uint16_t* rows_f16, int64_t n, const int32_t* lists);
int knnx_ivf_append(knnx_index* ix, const uint16_t* rows_f16, int64_t n, int32_t* lists_out);
int knnx_ivf_append_device(knnx_index* ix, const void* rows_dev_f16, int64_t n, int32_t* lists_out);
int knnx_ivf_merge_from(knnx_index* ix, knnx_index* other);
/* What the most recent of the four calls above that succeeded spent, for tools/ivf_append_bench.py: assign_ms = host time of the
 * assignment pass (0 where the caller named the lists), move_ms = device time of the arena move (payload copy, zero fill, idmap / inv), ids_ms = the idmap / inv pass alone (part of move_ms),
 * fill_ms = device time from the end of the move to the last scatter / encode kernel (for host rows it includes their upload),
 * moved_bytes = payload bytes the move copied (the occupied tiles of every arena; idmap / inv not counted).  Any pointer may be NULL.
 * KNNX_E_STATE before the first such call. */
int knnx_ivf_grow_stats(knnx_index* ix, double* assign_ms, double* move_ms, double* ids_ms, double* fill_ms, int64_t* moved_bytes);

/* ---- Shrinking a built index: faiss remove_ids (rows a safety filter flags, near-duplicate groups, take-down requests -- what
 * clip_back.py:326-341 filters per request because it treats the index file as frozen) ----
 * For the same indexes as the block above: every BUILT IVF index of any kind that owns its rows.  Ids here are POSITIONAL -- inv is a dense
 * table indexed by id - id_base, the list-ordered ids are a permutation of [0, ntotal), saved codes are kept in id order, metadata is
 * addressed by row number -- and a removal keeps all of that true: the survivors are renumbered densely in id order, as faiss'
 * IndexFlat.remove_ids does (faiss' IVF classes keep the old ids; on this point we differ on purpose).  After the call a surviving row with
 * old id o has id id_base + rank(o), rank(o) = the surviving ids below o.  Inside a list the survivors keep their order.  The layout is the
 * rule of knnx_ivf_begin applied to the new list sizes; pad rows are zero bytes in every payload and have idmap -1.  The result is, bit
 * for bit (arena, id maps, search results, exported codes, reconstructed rows, list-ordered ids), the index knnx_ivf_begin /
 * knnx_ivf_add_assigned / knnx_ivf_end build from the surviving rows in their original order with the same centroids, quantiser,
 * rotation, ranges and lists; of an IVF-Flat index the bound on the row norms is taken again over the survivors.
 *   knnx_ivf_remove_ids    ids host int64 [n], any order.  Entries that name no row -- -1, below id_base, at or above id_base + ntotal -- are
 *                          ignored (faiss' IDSelectorBatch), duplicates count once.  n_removed (may be NULL) receives the rows removed.
 *                          n == 0, or a call in which no id names a row, is a success that moves nothing, allocates nothing on the device
 *                          and leaves every cache as it was.  Removing every row is legal: it leaves ntotal == 0 and the one-tile arena of
 *                          an empty built index, every search answers with full padding, and knnx_ivf_append* works on it.  ids are
 *                          read in chunks of 2^20 through one staging buffer.
 * How: a flag per id is set (plain byte stores), a reduce-then-scan over the id space gives every survivor its new id (block sums scanned
 * on the host in int64), a ballot gives every source tile its 32-bit survivor mask, one wave per list turns the masks into the new list
 * sizes and into the destination row of every tile's first survivor, and a row-granular move copies the survivors of a source tile to
 * ONE contiguous run of the new arena; only the pad rows are zeroed.  The phases are separate launches: no kernel waits for another
 * workgroup.  The new sizes must add up to the survivors the id scan counted -- two independent device computations -- or the call answers
 * KNNX_E_STATE "internal: ..." before anything is swapped.  Like a growing call it is OUT OF PLACE, all or nothing and atomic for searchers:
 * new arena(s), idmap and inv next to the old ones (peak memory: old + new arena, plus 5 bytes per id and 8 per tile), swapped in at the
 * end under the lock the searches hold.  A flat index, an index between knnx_ivf_begin and knnx_ivf_end, borrowed rows, ids == NULL with
 * n > 0 and n < 0 answer KNNX_E_ARG with a message that ends in "nothing was removed", before anything is touched; an allocation that
 * fails answers KNNX_E_NOMEM with the index as it was.  nprobe, k_factor, the refine and threshold-scan switches, the counters, centroids
 * and quantiser are kept, and knnx_ivf_grow_stats keeps its answer.  The list-ordered ids change with every call that removes a row, so a
 * list-ordered metadata store must be exported again -- and the caller's embeddings and metadata rows must be filtered the same way, since
 * every id above the first removed one shifts.  An index handed to knnx_shards_adopt must not be shrunk afterwards (the shards' row ranges
 * would shift); a sharded removal is not provided. */
int knnx_ivf_remove_ids(knnx_index* ix, const int64_t* ids, int64_t n, int64_t* n_removed /* may be NULL */);
/* What the most recent knnx_ivf_remove_ids that succeeded spent, for tools/ivf_remove_bench.py: device time of the mark, plan (rank scan,
 * masks, list scan, layout; includes its host round trips), move (payload copy and pad rows) and ids (idmap / inv) phases; moved_bytes =
 * payload bytes of the survivors over every arena; n_removed.  A call that found nothing to remove reports zeros.  Any pointer may be
 * NULL.  KNNX_E_STATE before the first call. */
int knnx_ivf_remove_stats(knnx_index* ix, double* mark_ms, double* plan_ms, double* move_ms, double* ids_ms, int64_t* moved_bytes,
                          int64_t* n_removed);

/* Merge P per-shard results ([P, n, k] each, already global ids) into the top-k [n, k];
 * the step after the RCCL all-gather of a row-sharded index.  Device buffers.  k <= 64: any order within a list;
 * k > 64: every list sorted as knnx_search returns it (score descending, -1 padding at the tail), P <= 64. */
int knnx_merge_topk_device(int device, const float* D_parts, const int64_t* I_parts, int P, int n,
                           int k, float* D_out, int64_t* I_out, void* stream);

/* ---- one process, several GPUs: a row-sharded index behind ONE handle ----------------------------------------
 * `KnnService` keeps one index object per modality in one process and calls it from its request threads
 * (clip_back.py:343-362, 781-782, 1018); SURVEY 8(b) `knnx_create(n_devices, devices, ...)`, 8(e).  Shard g lives on
 * devices[g] (a device may be listed more than once) and holds the contiguous global row range [lo_g, hi_g), ids =
 * global row numbers.  A search sends the queries to every device, scans all shards concurrently (one stream per device),
 * copies the per-shard top-k (n*k*12 bytes) peer-to-peer over xGMI to devices[0] and merges there with the kernel of
 * knnx_merge_topk_device.  Same result contract as knnx_search.  Thread-safe (calls are serialised). */
typedef struct knnx_shards knnx_shards;
int knnx_shards_create(int n_shards, const int* devices, int d, int metric, knnx_shards** out);
/* Take ownership of per-device indexes built elsewhere (flat, IVF-Flat or IVF-PQ with replicated centroids -- and, IVF-PQ, the same
 * rotation or none; shard g must have been given id_base = row_lo[g]).  On success the shards are destroyed with the handle. */
int knnx_shards_adopt(int n_shards, knnx_index* const* shards, const int* devices, const int64_t* row_lo, knnx_shards** out);
void knnx_shards_destroy(knnx_shards* s);
/* Fix the row range of every shard (shard g = rows [g*T/G, (g+1)*T/G)) and size its arena; required before add. */
int knnx_shards_reserve(knnx_shards* s, int64_t total_rows);
/* faiss Index.add in global row order: fills shard 0, then shard 1, ... (streams to the owning shard). */
int knnx_shards_add_f16(knnx_shards* s, const uint16_t* rows, int64_t n);
int knnx_shards_add_f32(knnx_shards* s, const float* rows, int64_t n);
/* Benchmark corpus: shard g = knnx_synth_fill(rows_per_shard, seed + g), id_base = g * rows_per_shard. */
int knnx_shards_synth_fill(knnx_shards* s, int64_t rows_per_shard, uint64_t seed);
int64_t knnx_shards_ntotal(const knnx_shards* s);
int knnx_shards_count(const knnx_shards* s);
/* How the per-shard top-k lists reach devices[0]: 0 = hipMemcpyPeerAsync per shard (the default), 1 = one grouped ncclAllGather over
 * RCCL (opt-in: KNNX_SHARDS_RCCL=1 in the environment when the handle is created, every shard on its own device and librccl.so
 * loadable -- loaded with dlopen on first use; an exchange that fails switches the handle back to 0 and the batch is answered through
 * the peer copies), -1 = null handle.  Either way the same merge kernel produces the result. */
int knnx_shards_exchange(const knnx_shards* s);
knnx_index* knnx_shards_get(knnx_shards* s, int g); /* borrowed: profiling, nprobe */
/* faiss Index.search / search_and_reconstruct / reconstruct_batch / range_search over all shards. */
int knnx_shards_search(knnx_shards* s, const float* q, int n, int k, float* D, int64_t* I, float* R);
int knnx_shards_reconstruct(knnx_shards* s, const int64_t* ids, int64_t n, float* out);
int knnx_shards_range_search(knnx_shards* s, const float* q, int n, float thresh, int64_t* lims, float* D, int64_t* I);
/* List-ordered ids over all shards (the block "List-ordered ids" above): host arrays of knnx_shards_ntotal entries / n entries. */
int knnx_shards_id_order(knnx_shards* s, int64_t* old_to_new, int64_t* new_to_old);
int knnx_shards_map_ids(knnx_shards* s, const int64_t* ids, int64_t n, int64_t* out);

/* Counters of the proof-based scans (64-query wide scan, 256-query RQ scan): queries they served and queries whose
 * exactness proof failed and were re-run by the exact 32-query scan (each failure costs one more pass over HBM). */
int knnx_get_stats(knnx_index* ix, int64_t* proof_queries, int64_t* proof_failures);

/* IVF: number of 32-row tiles the most recent scan walked (the probed lists of its queries, padded to tiles; a call of more than
 * 32 queries is ONE multi-block pass of up to 256 -- every block of 32 walks the union of its own queries' lists, and the sum over
 * the blocks is reported); bytes read from HBM = tiles * 32 * d * 2, to be compared with (nprobe / nlist) * N * d * 2. */
int knnx_ivf_last_scan_tiles(knnx_index* ix, int64_t* tiles);
/* The same for the union over ALL queries of that pass (a list counted once however many blocks read it): the bytes one pass over
 * shared lists would read.  Collected only while profiling is enabled (knnx_profile_enable) during the search. */
int knnx_ivf_last_scan_union_tiles(knnx_index* ix, int64_t* tiles);

/* Live kernel timing for bench.py: when enabled, every scan launch is bracketed with
 * hipEvents on its own stream; get returns launches and summed milliseconds, then resets. */
int knnx_profile_enable(knnx_index* ix, int on);
int knnx_profile_get(knnx_index* ix, int64_t* scan_launches, double* scan_ms);

/* Fill n rows of an attached/reserved arena with the benchmark's synthetic corpus:
 * row r = L2-normalised N(0,1)^d from a counter-based hash of (seed, r, col), rounded to
 * fp16.  Re-derivable on the CPU (oracle/knn_oracle.py:synth_rows). */
int knnx_synth_fill(knnx_index* ix, int64_t n, uint64_t seed);

/* Benchmark corpora generated straight into caller HBM (fp16 [n, d]; dst row i = corpus row row_begin + i * row_stride; any row
 * is re-derivable on the CPU: oracle/knn_oracle.py).  kind 0: the isotropic corpus of knnx_synth_fill (row_stride 1 only);
 * kind 1: BASELINE config 5's overlapping mixture of n_clusters Gaussians in a 32-dimensional latent space, where IVF recall
 * is < 1 at small nprobe and rises with it; kind 2: the isotropic corpus with three dominant columns (6 x the spread plus a common
 * offset, as a few dimensions of real CLIP embeddings have: the int8 first stage treats them as dominant columns, knnx_i8_dominant;
 * row_stride 1 only).
 * `stream`: hipStream_t or NULL; synchronous. */
int knnx_synth_rows_device(int device, void* dst_f16, int64_t row_begin, int64_t row_stride, int64_t n, int d, uint64_t seed,
                           int kind, int64_t n_clusters, void* stream);

/* ---- request coalescing ("knnx_search is re-entrant; internally a batching queue") ---------------------------
 * The service calls the index from concurrent request threads with ONE query each (clip_back.py:1018 -> :362).  With coalescing
 * on (the default), knnx_search calls with n == 1 and k <= 64 that arrive while the GPU is busy wait in a queue inside the
 * library; the first caller to find no leader serves everything queued with the same k -- up to one scan's worth, 256 queries --
 * in ONE pass over HBM (one batched gather for the callers that want R), hands each caller its slice and passes the lead on.
 * Results are those of the uncoalesced call: the same ids, scores equal to f32 summation order (the scan kernel that serves a
 * query depends on how many queries share its pass).  Calls with n > 1 or
 * k > 64 are served directly.  knnx_set_coalesce(ix, 0) turns the queue off; knnx_coalesce_stats: batches served, queries in
 * them, the largest batch so far (any pointer may be NULL). */
int knnx_set_coalesce(knnx_index* ix, int on);
int knnx_coalesce_stats(knnx_index* ix, int64_t* batches, int64_t* queries, int64_t* largest_batch);

/* int8 first stage of the flat scans (round 4; no counterpart in the reference: faiss IndexFlatIP scans its one copy of the rows,
 * clip_back.py:362).  A flat (non-IVF) index of d = 512 / 768 / 1024 with at least 2^21 rows keeps, when the memory can be had,
 * an int8 copy of its fp16 rows (one scale per column) and scans THAT with 1 .. 256 queries per pass -- half the bytes, int8 MFMA --
 * to decide which rows are re-scored exactly from the fp16 rows; the admission threshold carries a proven bound of the quantisation
 * error (every fp32 norm in it widened by 1 + 1e-3, which covers its own rounding with an order of magnitude to spare), so D and I
 * are the exact top-k as without it (a query whose hit list overflows is re-run by the exact scan).  The copy is
 * built on the first search after the rows changed (one pass over the rows) and costs ntotal * d bytes; KNNX_I8=0 in the environment
 * turns it off.  When ntotal * d bytes cannot be had next to the rows (the headline shard: 125 M x 768 fp16 = 192 GB of a 288 GB part)
 * or KNNX_I8_MAX_BYTES caps it, the copy is PARTIAL: it holds as many leading rows as fit (at least a quarter of the index, else
 * none), those get the int8 first stage and the rows behind them are scanned in fp16 into the same hit lists -- one proof, one
 * result.  Any later allocation of the index that fails takes the copy's memory back and turns the feature off.
 * knnx_i8_served: queries answered through this path so far (-1: null index); knnx_i8_rows: rows the copy holds now (0: none). */
int64_t knnx_i8_served(knnx_index* ix);
int64_t knnx_i8_rows(knnx_index* ix);
/* 0: no int8 copy at the moment; 1 / 2: int8 planes per query.  A query is quantised as u = q * (column scales) with ONE scale, so an
 * index with a few columns much larger than the rest ("dominant": column scale > 3 x the median one; CLIP embeddings have them)
 * would leave the other components in the rounding error and admit (and re-score) two orders of magnitude more rows.  Decided at
 * every full build of the copy:
 *   no dominant column:  one plane
 *   1 .. 4 of them:      one plane; the copy keeps those columns in bytes 0..3 of each row (its layout is private), the matrix product
 *                        leaves them out and the scan adds their part with 14-bit query digits on the vector ALU (round 5) -- the
 *                        speed of one plane, 256 queries per pass.  knnx_i8_dominant: how many, and which columns (cols4: room for
 *                        4 ints, may be NULL); 0 when the index has none or the form is off (KNNX_I8_DOM=0 in the environment)
 *   more:                a second plane for what the first left -- twice the matrix work, four waves x 32 queries per pass
 * KNNX_I8_PLANES=1|2 forces the plane count (and switches the dominant-column form off). */
int knnx_i8_planes(knnx_index* ix);
int knnx_i8_dominant(knnx_index* ix, int* cols4);

/* One request of KnnService.knn_search with its dedup fused (clip_back.py:362 + :290-309): the top-k (k <= 64) of ONE query, and
 * the links of the reference's `get_non_uniques` -- every pair of result ranks (i < j) whose stored vectors, L2-normalised in
 * f32 as `normalized()` does (clip_back.py:194-197, :378), have inner product > dedup_thr (the reference: 0.94, strict).  The
 * k result rows are gathered ONCE on the device for the whole coalesced batch and the links of all its requests come from one
 * launch; they need not travel to the host (R_or_null = NULL).  pairs: int32 [2 * pairs_cap] = (i0, j0, i1, j1, ...), sorted;
 * *n_pairs = number of links found -- when it exceeds pairs_cap (or 512) only the first are stored and the caller should take
 * the general path (knnx_reconstruct + knnx_range_search_once).  Connected components over the links are the caller's. */
int knnx_search_dedup(knnx_index* ix, const float* q, int k, float* D, int64_t* I, float* R_or_null, float dedup_thr,
                      int32_t* pairs, int pairs_cap, int* n_pairs);

/* ---- Post filter on the device: one request of any k <= 8192 with its dedup, violence and safety filters where the rows are ---------
 * KnnService.knn_search asks for 3 000 results with all three filters (clip_back.py:343-399).  knnx_search_filtered answers ONE query:
 * the search, one gather of the result rows into device scratch, and the three filters there; D, I and one byte per result come back.
 *
 * Search:    D, I are exactly what knnx_search(ix, q, 1, k, D, I, NULL) returns for this index -- flat, IVF-Flat, IVF-PQ in all its
 *            variants, IVF-SQ8; the compressed families keep their k > 64 rule and answer as knnx_search does while their threshold
 *            scan is off.  n = the number of leading results with id >= 0; drop[n .. k-1] = 0.
 * Rows:      r_i = the f32 row knnx_reconstruct returns for I[i], the same bits (IVF-PQ: decoded and back-rotated, or the refine
 *            store's row where there is one; IVF-SQ8: decoded).
 * Normalise: as normalized() does (clip_back.py:194-197): s_i = one fmaf chain over the columns 0 .. d_user-1 in ascending order from
 *            +0, e_i[c] = r_i[c] / sqrtf(s_i); a row with s_i == 0 stays 0.  Columns d_user .. d-1 of an index row are the zero padding
 *            the Python layer adds and take no part.  d_user <= d, and every MLP's input width must equal d_user: KNNX_E_ARG otherwise,
 *            the message names both numbers.
 * Dedup      (dedup_on != 0; clip_back.py:290-309): sim(i, j) = one fmaf chain over c ascending of e_i[c] * e_j[c] from +0 (what
 *            v_mfma_f32_32x32x2_f32 computes).  Ranks i < j are linked iff sim > dedup_thr (strict); every rank that is not the
 *            smallest member of its connected component gets KNNX_DROP_DUPLICATE.  The links are counted (stats->n_links), never
 *            returned; the device keeps 2^20 of them: a request with more sets stats->links_overflowed = 1, sets NO duplicate bit at
 *            all and still fills the other two -- the caller then takes the general path for dedup (knnx_reconstruct +
 *            knnx_range_search_once).  Call with stats when dedup is on.
 * Violence   (violence_or_null; clip_back.py:326-331): a bias-free one-layer knnx_mlp [P, d_user] holding the prompt embeddings;
 *            KNNX_DROP_VIOLENT iff the FIRST maximum of the P scores of e_i is prompt 1.
 * Safety     (safety_or_null; clip_back.py:315-325): KNNX_DROP_UNSAFE iff output 0 of the MLP on e_i is > safety_thr.
 * Refused before anything is launched: k > KNNX_FILTER_MAX_K (KNNX_E_UNSUPPORTED, names the limit); an MLP that lives on another
 * device than the index (KNNX_E_ARG); no filter asked for (KNNX_E_ARG: knnx_search is the call for that).
 * The call takes the index once for search, gather and filter, on the index's stream; it is not coalesced with other requests.
 * Deterministic: the same drop bytes for the same index and query, alone or beside other threads.  stats->cc_rounds: rounds of the
 * connected-components kernel (0: it had nothing to do); more than n of them cannot happen and would answer KNNX_E_STATE. */
#define KNNX_FILTER_MAX_K 8192
#define KNNX_DROP_DUPLICATE 1
#define KNNX_DROP_VIOLENT 2
#define KNNX_DROP_UNSAFE 4
typedef struct {
  int32_t n_valid, n_links, links_overflowed, cc_rounds;
} knnx_filter_stats;
typedef struct knnx_mlp knnx_mlp; /* the resident fp32 MLP of the block below */
int knnx_search_filtered(knnx_index* ix, const float* q, int k, int d_user, int dedup_on, float dedup_thr,
                         knnx_mlp* violence_or_null, knnx_mlp* safety_or_null, float safety_thr, float* D, int64_t* I,
                         uint8_t* drop, knnx_filter_stats* stats_or_null);

/* ---- post filter: the safety head on the GPU --------------------------------------------------------
 * Replaces `safety_model.predict(embeddings, batch_size)` of clip_retrieval/clip_back.py:315-325 for a model that is a stack
 * of fp32 Linear layers with ReLU between them -- the H14 detector of clip_retrieval/h14_nsfw_model.py:16-34
 * (1024 -> 1024 -> 2048 -> 1024 -> 256 -> 128 -> 16 -> 1, Dropout = identity in eval mode).  dims: n_layers + 1 widths;
 * weights[l]: f32 [dims[l+1], dims[l]] row-major (torch.nn.Linear.weight), biases[l]: f32 [dims[l+1]] or NULL;
 * relu[l] != 0: ReLU after layer l (NULL: after every layer but the last).  fp32 FMA, f32 accumulate in k order. */
int knnx_mlp_create(int device, int n_layers, const int32_t* dims, const float* const* weights, const float* const* biases,
                    const uint8_t* relu, knnx_mlp** out);
/* x: host f32 [n, dims[0]] -> y: host f32 [n, dims[n_layers]]; synchronous; calls on one handle are serialised. */
int knnx_mlp_forward(knnx_mlp* m, const float* x_host, int n, float* y_host);
/* The same layers applied to n rows that are already on the handle's device: x_dev f32, row r at x_dev + r * ld (ld >= dims[0]) ->
 * y_dev f32 [n, dims[n_layers]], left on the device.  The bits equal those of knnx_mlp_forward on the same inputs (the same kernel,
 * a k-ordered fmaf chain from 0 plus the bias).  stream: a hipStream_t of that device, NULL: the handle's own.  Holds the handle's
 * mutex until its kernels have completed on `stream` (the layers share the handle's activation buffers), so it is synchronous too. */
int knnx_mlp_forward_device(knnx_mlp* m, const float* x_dev, int64_t ld, int n, float* y_dev, void* stream);
int knnx_mlp_device(const knnx_mlp* m); /* the device the handle lives on, -1: null */
int knnx_mlp_destroy(knnx_mlp* m);

const char* knnx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* KNNX_H */
