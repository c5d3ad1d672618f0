"""The small corpus the device-builder trace test and the three-routes test share: 5000 x 256 rows of the benchmark's mixture
(n % 32 != 0, and with chunk = 2000 a ragged last chunk), produced on the device by the generator that also serves as `fill_rows`,
with a given coarse quantiser of 16 lists and given PQ (M = 16) / SQ8 quantisers."""
import numpy as np

N, D, NLIST, CHUNK, M = 5000, 256, 16, 2000, 16
SEED, CLUSTERS = 11, 24

_CACHE = {}


def fill_rows(dst_ptr, row0, count, stride):
    """fill_rows of the device builders: rows row0, row0 + stride, ... of the corpus at dst_ptr (complete when it returns)."""
    import torch

    from clip_retrieval_amd.knn import synth_rows_device

    synth_rows_device(dst_ptr, row0, count, D, SEED, kind=1, n_clusters=CLUSTERS, row_stride=stride, device=0)
    torch.cuda.synchronize(0)


def corpus():
    """dict(x fp16 [N, D], cent fp16 [NLIST, D], codebooks f32 [M, 256, D / M], ranges (vmin, vdiff) f32 [D], rotation f32 [D, D],
    rect f32 [2 D, D] with orthonormal columns, q f32 [8, D]) -- computed once and shared; nobody changes it."""
    import torch

    from clip_retrieval_amd.knn import opq_initial_rotation

    if not _CACHE:
        t = torch.empty((N, D), dtype=torch.float16, device="cuda:0")
        fill_rows(t.data_ptr(), 0, N, 1)
        x = t.cpu().numpy()
        rng = np.random.default_rng(SEED)
        x32 = x.astype(np.float32)
        cent = x32[np.sort(rng.choice(N, NLIST, replace=False))]
        cent = (cent / np.linalg.norm(cent, axis=1, keepdims=True)).astype(np.float16)
        codebooks = (0.04 * rng.standard_normal((M, 256, D // M))).astype(np.float32)
        vmin = x32.min(0)
        q = x32[rng.integers(0, N, 8)] + 0.02 * rng.standard_normal((8, D)).astype(np.float32)
        _CACHE.update(x=x, cent=cent, codebooks=codebooks, ranges=(vmin, x32.max(0) - vmin), rotation=opq_initial_rotation(D, SEED),
                      rect=np.ascontiguousarray(opq_initial_rotation(2 * D, SEED)[:, :D]),
                      q=np.ascontiguousarray(q, dtype=np.float32))
        for v in (x, cent, codebooks, vmin, _CACHE["ranges"][1], _CACHE["rotation"], _CACHE["rect"], _CACHE["q"]):
            v.setflags(write=False)
    return _CACHE
