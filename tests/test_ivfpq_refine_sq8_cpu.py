"""The parts of the SQ8 refine store of IVF-PQ that need no device: the index key and the manifest."""
import numpy as np
import pytest

from clip_retrieval_amd.knn import IVFPQ_REFINE_RANGES, ivfpq_params_from_index_key, read_ivfpq_refine_kind


@pytest.mark.parametrize("key,d,refine", [  # (None: refused, as before)
    ("IVF4096,PQ64x8,Refine(SQ8)", 1024, "sq8"), ("OPQ256_768,IVF16384_HNSW32,PQ256x8,Refine(SQ8)", 512, "sq8"),
    ("IVF4096,PQ64x8,RFlat", 1024, True), ("IVF4096,PQ64x8", 1024, False),
    ("IVF4096,PQ64x8,Refine(Flat)", 1024, None), ("IVF4096,PQ64x8,Refine(SQ8),RFlat", 1024, None)])
def test_index_key_names_the_store(key, d, refine):
    if refine is None:
        with pytest.raises(ValueError, match="not served"):
            ivfpq_params_from_index_key(key, d)
    else:
        assert ivfpq_params_from_index_key(key, d)["refine"] == refine


def test_manifest_kind(tmp_path):
    """Without "refine_kind" a manifest is what it always was; "sq8" needs "refine": true and its sidecar [2, d], the sidecar the key."""
    rng = np.arange(512, dtype=np.float32).reshape(2, 256)
    f, sq8 = str(tmp_path), {"d": 256, "refine": True, "refine_kind": "sq8"}
    assert read_ivfpq_refine_kind(f, {"d": 256}) is False and read_ivfpq_refine_kind(f, {"d": 256, "refine": True}) is True
    np.save(tmp_path / IVFPQ_REFINE_RANGES, rng)
    kind, (vmin, vdiff) = read_ivfpq_refine_kind(f, sq8)
    assert kind == "sq8" and np.array_equal(vmin, rng[0]) and np.array_equal(vdiff, rng[1])
    for bad in ({"d": 256, "refine_kind": "sq8"}, {**sq8, "refine_kind": "sq4"}, {"d": 256, "refine": True}, {**sq8, "d": 512}):
        with pytest.raises(ValueError):
            read_ivfpq_refine_kind(f, bad)
