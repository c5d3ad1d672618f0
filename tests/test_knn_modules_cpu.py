"""The kNN Python layer is four modules behind one public face: `knn` keeps every name it ever exported, and the modules import one way
only (knn_index <- knn_train <- knn_build <- knn_store)."""
import ast
import os

CHAIN = ["knn_index", "knn_train", "knn_build", "knn_store"]
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clip-retrieval_amd")

# every class, function and constant that `clip-retrieval_amd/knn.py` defined while it was one file, plus what it imported from _lib
NAMES = """
HipLibraryError check load_library METRIC_INNER_PRODUCT _SCAN_QUERIES _as_queries _map_ids_call _threshold_scan_property _threshold_stats
_own_handle _shard_handles _FaissShaped Mi355xIndex ShardedMi355xIndex get_old_to_new_mapping search_to_new_ids embedding_files load_index
IvfBuilder synth_rows_device rebalance_centroids train_ivf_centroids_device _download_i32 _release_cached_device_memory
build_ivf_index_device train_ivf_centroids _positions_in_lists _list_sizes _ivf_begin _add_assigned_chunks _add_code_chunks _ivf_end
_encode_chunks _split_saved_rows threshold_scan_entry read_threshold_scan ivfpq_threshold_scan_entry ivfsq_threshold_scan_entry
read_ivfpq_threshold_scan read_ivfsq_threshold_scan build_ivf_index IVF_MANIFEST IVF_FORMAT FolderRows _scatter_into_ivf _remember_folder
append_new_folder_rows build_ivf_index_from_folder save_index read_ivf_manifest _load_ivf_index PQ_SAMPLE_ROWS IVFPQ_MANIFEST
IVFPQ_ROTATION IVFPQ_FORMAT _f16_padded PqBuilder train_pq_codebooks OPQ_SAMPLE_ROWS _pad_rotation rotate_rows_device rotate_rows
opq_procrustes opq_initial_rotation train_opq_device opq_embedding _check_opq_dim train_opq _resolve_rotation _rotation_out_dim train_ivfpq
ivfpq_params_from_index_key _ivfpq_begin _ivfpq_encode_chunks _assign_chunks build_ivfpq_index build_ivfpq_index_from_folder
build_ivfpq_index_device _save_ivfpq_index ivfpq_out_dim_entry read_ivfpq_out_dim read_ivfpq_rotation read_ivfpq_refine
_ivfpq_refine_from_rows _ivfpq_from_codes _load_ivfpq_index IVFSQ_MANIFEST IVFSQ_FORMAT train_sq_ranges ivfsq_params_from_index_key
ivfsq_manifest check_ivfsq_manifest _ivfsq_begin _ivfsq_encode_chunks build_ivfsq_index build_ivfsq_index_from_folder
build_ivfsq_index_device _save_ivfsq_index _ivfsq_from_codes _load_ivfsq_index
""".split()


def test_knn_still_exports_every_name():
    from clip_retrieval_amd import knn  # (imports without a GPU)

    missing = [n for n in NAMES if not hasattr(knn, n)]
    assert not missing, f"no longer importable from clip_retrieval_amd.knn: {missing}"
    assert knn.ivfpq_threshold_scan_entry is knn.threshold_scan_entry and knn.read_ivfsq_threshold_scan is knn.read_threshold_scan


def _imported_knn_modules(name):
    with open(os.path.join(PKG, name + ".py"), encoding="utf-8") as f:
        tree = ast.parse(f.read())
    out = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.module:
            out.add(node.module.split(".")[-1])
            out.update(a.name for a in node.names)  # (from . import knn_build)
        elif isinstance(node, ast.Import):
            out.update(a.name.split(".")[-1] for a in node.names)
    return {m for m in out if m == "knn" or m in CHAIN}


def test_knn_modules_import_one_way():
    for i, name in enumerate(CHAIN):
        later = _imported_knn_modules(name) & (set(CHAIN[i:]) | {"knn"})
        assert not later, f"{name} imports {sorted(later)}: a module of the chain imports only earlier ones, and never knn"
    assert _imported_knn_modules("knn") == set(CHAIN)
    with open(os.path.join(PKG, "knn.py"), encoding="utf-8") as f:
        assert not any(isinstance(n, ast.ImportFrom) and any(a.name == "*" for a in n.names) for n in ast.walk(ast.parse(f.read())))
