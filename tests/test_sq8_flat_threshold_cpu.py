"""The threshold scan of flat SQ8 (k > 64 and range_search behind Mi355xIndex.sq8_threshold_scan) without a GPU: the three symbols answer
before any HIP call, and the saved manifest carries the switch only when it is on."""
import ctypes as C
import json

import pytest


def test_symbols_answer_without_hip():
    from clip_retrieval_amd._lib import load_library

    lib = load_library()
    KNNX_E_ARG = lib.knnx_add_f16(None, None, C.c_int64(1))  # the argument error of every entry point
    assert KNNX_E_ARG != 0 and lib.knnx_sq8_threshold_scan(None) == 0
    assert lib.knnx_sq8_set_threshold_scan(None, 1) == KNNX_E_ARG and lib.knnx_sq8_threshold_stats(None, None, None, None, None) == KNNX_E_ARG


def test_manifest_carries_the_switch_only_when_on(tmp_path):
    from clip_retrieval_amd import knn_store as ks

    off = ks.flat_sq8_manifest(768, (100, 1137))
    assert "threshold_scan" not in {**off, **ks.threshold_scan_entry(False)} and ks.read_threshold_scan("x", off) is False
    on = ks._write_manifest(str(tmp_path), ks.FLAT_SQ8_MANIFEST, {**off, **ks.threshold_scan_entry(True)})  # pylint: disable=protected-access
    assert json.loads((tmp_path / ks.FLAT_SQ8_MANIFEST).read_text(encoding="utf-8")) == {**off, "threshold_scan": True} == on
    back = ks.check_flat_sq8_manifest(ks._read_manifest(str(tmp_path), ks.FLAT_SQ8_MANIFEST), "x")  # pylint: disable=protected-access
    assert back == on and ks.read_threshold_scan("x", back) is True
    for bad in (1, "true", None):
        with pytest.raises(ValueError, match="threshold_scan"):
            ks.check_flat_sq8_manifest({**off, "threshold_scan": bad}, "x")
