// knnx_filter.hip -- knnx_search_filtered: one request of any k <= KNNX_FILTER_MAX_K with its dedup, violence and safety filters run
// where the result rows already are (include/knnx.h, "Post filter on the device").  Kernels: knn_filter_kernels.hip; the
// integer arithmetic both share: knnx_filter_plan.h.  Written to the rules of DESIGN 3.1: refusals before the first launch, one
// all-or-nothing scratch group (FilterScratch), ix->mu taken once, everything on ix->stream, one synchronisation point per hand-over.
#include "knnx_host.h"

static int mlp_check(const knnx_index* ix, knnx_mlp* m, const char* what, int d_user, bool one_bias_free_layer, int* d_out) {
  int d_in = 0, layers = 0, bias = 0;
  knnx_mlp_shape(m, &d_in, d_out, &layers, &bias);
  if (knnx_mlp_device(m) != ix->device)
    return fail(KNNX_E_ARG, std::string("search_filtered: the ") + what + " model lives on device " + std::to_string(knnx_mlp_device(m)) +
                                ", the index on device " + std::to_string(ix->device));
  if (d_in != d_user)
    return fail(KNNX_E_ARG, std::string("search_filtered: the ") + what + " model takes " + std::to_string(d_in) + " inputs, d_user is " +
                                std::to_string(d_user));
  if (one_bias_free_layer && (layers != 1 || bias))
    return fail(KNNX_E_ARG, std::string("search_filtered: the ") + what + " model must be ONE bias-free layer [P, d_user] (the prompt embeddings)");
  return KNNX_OK;
}

extern "C" int knnx_search_filtered(knnx_index* ix, const float* q, int k, int d_user, int dedup_on, float dedup_thr,
                                    knnx_mlp* violence, knnx_mlp* safety, float safety_thr, float* D, int64_t* I, uint8_t* drop,
                                    knnx_filter_stats* stats) {
  if (k > KNNX_FILTER_MAX_K)
    return fail(KNNX_E_UNSUPPORTED, "search_filtered serves k <= " + std::to_string(KNNX_FILTER_MAX_K) + " (KNNX_FILTER_MAX_K), got " +
                                        std::to_string(k));
  if (!ix || !q || !D || !I || !drop || k <= 0) return fail(KNNX_E_ARG, "bad search_filtered arguments");
  if (!dedup_on && !violence && !safety) return fail(KNNX_E_ARG, "search_filtered: no filter asked for (knnx_search is the call for that)");
  if (d_user <= 0 || d_user > ix->d)
    return fail(KNNX_E_ARG, "search_filtered: d_user = " + std::to_string(d_user) + " must be in [1, d = " + std::to_string(ix->d) + "]");
  if (ix->d % 4 || ix->d > 4096)
    return fail(KNNX_E_UNSUPPORTED, "search_filtered needs d % 4 == 0 and d <= 4096, the index has d = " + std::to_string(ix->d));
  int v_out = 0, s_out = 0, r = 0;
  if (violence && (r = mlp_check(ix, violence, "violence", d_user, true, &v_out))) return r;
  if (safety && (r = mlp_check(ix, safety, "safety", d_user, false, &s_out))) return r;
  if (stats) *stats = knnx_filter_stats{0, 0, 0, 0};

  std::lock_guard<std::mutex> lk(ix->mu);
  if (set_dev(ix)) return KNNX_E_HIP;
  hipStream_t st = ix->stream;
  // 1. the search, as knnx_search runs it for host buffers (its refusals included); D and I are final after this
  if ((r = search_locked(ix, q, 1, k, D, I))) return r;
  int n = 0;
  while (n < k && I[n] >= 0) ++n;
  memset(drop, 0, (size_t)k);
  if (stats) stats->n_valid = n;
  if (n == 0) return KNNX_OK;

  // 2. scratch: everything or nothing, before the first launch of the filter
  FilterScratch& F = ix->filter;
  const hipError_t ae = F.alloc(ix, k, v_out, s_out);
  if (ae != hipSuccess) {
    (void)hipGetLastError();
    return fail(KNNX_E_NOMEM, "search_filtered: " + std::to_string(filter_sizes(k, ix->d, v_out, s_out).bytes()) +
                                  " bytes of filter scratch could not be had: " + hipGetErrorString(ae));
  }
  const size_t ids_b = (size_t)k * sizeof(int64_t), cnt_b = FILTER_COUNTERS * sizeof(int);
  if ((r = ensure_pin(ix, ids_b + cnt_b + (size_t)k))) return r;
  int64_t* ids_pin = (int64_t*)ix->pin.p;
  int* cnt_pin = (int*)((char*)ix->pin.p + ids_b);
  uint8_t* drop_pin = (uint8_t*)((char*)ix->pin.p + ids_b + cnt_b);
  if (scratch_acquire(ix, st)) return KNNX_E_HIP;

  // 3. the rows of the n results, once, by the kernels of knnx_reconstruct; unit rows in place
  memcpy(ids_pin, I, (size_t)n * sizeof(int64_t));
  HIPCHK(hipMemcpyAsync(F.ids, ids_pin, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(F.counters, 0, cnt_b, st));
  if (ix->pq.m) {
    if ((r = pq_decode_rows(ix, F.ids, n, F.rows, st))) return r;
  } else if (ix->sq.on) {
    if ((r = sq_decode_rows(ix, F.ids, n, F.rows, st))) return r;
  } else if (ix->ivf_nlist) {
    HIPCHK(launch_gather_inv(ix->rows, ix->d, ix->id_base, ix->ntotal, ix->ivf.inv, F.ids, n, F.rows, st));
  } else {
    HIPCHK(launch_gather(ix->rows, ix->ntotal, ix->d, ix->id_base, F.ids, n, F.rows, st));
  }
  HIPCHK(launch_filter_normalise(F.rows, n, ix->d, d_user, st));

  // 4. links (asynchronous; the two heads below run behind them on the same stream), scores, bits, components
  if (dedup_on) HIPCHK(launch_filter_links(F.rows, n, ix->d, d_user, dedup_thr, F.links, (int)FILTER_LINK_CAP, F.counters, st));
  if (violence && (r = knnx_mlp_forward_device(violence, F.rows, ix->d, n, F.vscores, st))) return r;
  if (safety && (r = knnx_mlp_forward_device(safety, F.rows, ix->d, n, F.sscores, st))) return r;
  HIPCHK(launch_filter_bits(violence ? (const float*)F.vscores : nullptr, v_out, safety ? (const float*)F.sscores : nullptr, s_out, safety_thr, n, k,
                            F.drop, st));
  if (dedup_on) HIPCHK(launch_filter_cc(F.links, (int)FILTER_LINK_CAP, F.counters, n, F.drop, st));

  // 5. one byte per result and the counters come back
  HIPCHK(hipMemcpyAsync(drop_pin, F.drop, (size_t)k, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(cnt_pin, F.counters, cnt_b, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (scratch_release(ix, st)) return KNNX_E_HIP;
  if (cnt_pin[FILTER_C_BOUND])
    return fail(KNNX_E_STATE, "internal: the connected-components rounds did not end within their bound of " + std::to_string(n));
  memcpy(drop, drop_pin, (size_t)k);
  if (stats) {
    stats->n_links = cnt_pin[FILTER_C_LINKS];
    stats->links_overflowed = cnt_pin[FILTER_C_LINKS] > FILTER_LINK_CAP ? 1 : 0;
    stats->cc_rounds = cnt_pin[FILTER_C_ROUNDS];
  }
  return KNNX_OK;
}
