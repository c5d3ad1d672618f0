"""Flat SQ8 without a GPU: the new symbols answer before any HIP call, the manifest of a saved folder round-trips and a damaged one is
refused, and knn re-exports the new names through the one-way import chain."""
import ctypes as C
import json

import numpy as np
import pytest


def test_symbols_answer_without_hip():
    from clip_retrieval_amd._lib import load_library

    lib = load_library()
    assert lib.knnx_sq8(None) == 0
    v = np.zeros(256, dtype=np.float32)
    KNNX_E_ARG = lib.knnx_add_f16(None, None, C.c_int64(1))  # the argument error of every entry point
    assert KNNX_E_ARG != 0 and lib.knnx_sq8_set_quantizer(None, v.ctypes.data, v.ctypes.data) == KNNX_E_ARG
    assert b"sq8_set_quantizer" in lib.knnx_last_error()
    for fn in (lib.knnx_sq8_get_quantizer, lib.knnx_sq8_add_codes, lib.knnx_sq8_add_device_f16, lib.knnx_sq8_get_codes):
        assert callable(fn)


def test_manifest_round_trip_and_refusals(tmp_path):
    from clip_retrieval_amd import knn_store as ks

    man = ks._write_manifest(str(tmp_path), ks.FLAT_SQ8_MANIFEST, ks.flat_sq8_manifest(768, (100, 1137)))
    back = ks.check_flat_sq8_manifest(ks._read_manifest(str(tmp_path), ks.FLAT_SQ8_MANIFEST), "x")
    assert back == man == {"format": ks.FLAT_SQ8_FORMAT, "kind": "flat_sq8", "d": 768, "row_range": [100, 1137]}
    for damage in ({"format": ks.IVFSQ_FORMAT}, {"kind": "ivfsq"}, {"d": 0}, {"d": "768"}, {"row_range": [5, 1]}, {"row_range": [0]}):
        with pytest.raises(ValueError, match="flat SQ8 manifest"):
            ks.check_flat_sq8_manifest({**man, **damage}, "x")
    ok = (np.zeros(768, np.float32), np.ones(768, np.float32), np.zeros((1037, 768), np.uint8))
    ks.check_flat_sq8_files(man, *ok, "x")
    for i, bad in ((0, np.zeros(512, np.float32)), (1, np.ones(768, np.float64)), (2, np.zeros((1036, 768), np.uint8)),
                   (2, np.zeros((1037, 768), np.int8))):
        with pytest.raises(ValueError, match="disagree with the manifest"):
            ks.check_flat_sq8_files(man, *[bad if j == i else a for j, a in enumerate(ok)], "x")
    (tmp_path / ks.FLAT_SQ8_MANIFEST).write_text(json.dumps({"format": "other"}))
    with pytest.raises(ValueError, match="flat SQ8 manifest"):
        ks.load_index(str(tmp_path))


def test_knn_exports_and_import_chain():
    from clip_retrieval_amd import knn, knn_build, knn_index, knn_store, knn_train

    for name in ("build_sq8_index", "build_sq8_index_device", "flat_sq8_manifest", "check_flat_sq8_manifest", "FLAT_SQ8_MANIFEST"):
        assert hasattr(knn, name), name
    assert isinstance(knn.Mi355xIndex.is_sq8, property) and callable(knn.Mi355xIndex.set_sq8_quantizer)
    mods = [knn_index, knn_train, knn_build, knn_store]
    for i, m in enumerate(mods):  # a module never holds a later module of the chain
        for later in mods[i + 1:]:
            assert later not in vars(m).values(), f"{m.__name__} imports {later.__name__}"
