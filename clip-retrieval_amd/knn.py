"""The public face of the kNN half: faiss-`Index`-shaped objects over the MI355X kNN library, their builders and their folders.

The code lives in four modules, one per concern, that import one way only (knn_index <- knn_train <- knn_build <- knn_store):
  * knn_index   Mi355xIndex / ShardedMi355xIndex -- the part of the faiss Index API the reference exercises -- and the
                reference-named id-order helpers;
  * knn_train   the device trainers: k-means, PQ codebooks, the OPQ rotation, SQ8 ranges; the index-key parsers;
  * knn_build   {IVF-Flat, IVF-PQ, IVF-SQ8} x {host array, embeddings folder, rows produced on the GPU} over two drivers;
  * knn_store   save_index / load_index and the three folder formats (`load_index` takes the place of clip_back.py:589-596).
Everything that could be imported from this module still can; the underscore names are the ones tests and tools reach for.
"""

# pylint: disable=unused-import
from ._lib import HipLibraryError, check, load_library
from .knn_build import (FolderRows, _add_assigned_chunks, _assign_chunks, _download_i32, _encode_chunks, _ivf_begin, _ivf_end, _ivfpq_begin,
                        _ivfpq_encode_chunks, _ivfsq_begin, _ivfsq_encode_chunks, _list_sizes, _positions_in_lists,
                        _release_cached_device_memory, _remember_folder, _scatter_into_ivf, append_new_folder_rows, build_ivf_index,
                        build_ivf_index_device, build_ivf_index_from_folder, build_ivfpq_index, build_ivfpq_index_device,
                        build_ivfpq_index_from_folder, build_ivfsq_index, build_ivfsq_index_device, build_ivfsq_index_from_folder,
                        embedding_files)
from .knn_index import (_SCAN_QUERIES, METRIC_INNER_PRODUCT, Mi355xIndex, ShardedMi355xIndex, _as_queries, _FaissShaped, _map_ids_call,
                        _own_handle, _pad_rotation, _shard_handles, _threshold_scan_property, _threshold_stats, get_old_to_new_mapping,
                        search_to_new_ids)
from .knn_store import (IVF_FORMAT, IVF_MANIFEST, IVFPQ_FORMAT, IVFPQ_MANIFEST, IVFPQ_ROTATION, IVFSQ_FORMAT, IVFSQ_MANIFEST,
                        _add_code_chunks, _ivfpq_from_codes, _ivfpq_refine_from_rows, _ivfsq_from_codes, _load_ivf_index, _load_ivfpq_index,
                        _load_ivfsq_index, _save_ivfpq_index, _save_ivfsq_index, _split_saved_rows, check_ivfsq_manifest, ivfpq_out_dim_entry,
                        ivfpq_threshold_scan_entry, ivfsq_manifest, ivfsq_threshold_scan_entry, load_index, read_ivf_manifest,
                        read_ivfpq_out_dim, read_ivfpq_refine, read_ivfpq_rotation, read_ivfpq_threshold_scan, read_ivfsq_threshold_scan,
                        read_threshold_scan, save_index, threshold_scan_entry)
from .knn_train import (OPQ_SAMPLE_ROWS, PQ_SAMPLE_ROWS, IvfBuilder, PqBuilder, _check_opq_dim, _f16_padded, _resolve_rotation,
                        _rotation_out_dim, ivfpq_params_from_index_key, ivfsq_params_from_index_key, opq_embedding, opq_initial_rotation,
                        opq_procrustes, rebalance_centroids, rotate_rows, rotate_rows_device, synth_rows_device, train_ivf_centroids,
                        train_ivf_centroids_device, train_ivfpq, train_opq, train_opq_device, train_pq_codebooks, train_sq_ranges)
