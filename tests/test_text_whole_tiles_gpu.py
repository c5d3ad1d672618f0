"""Ragged text batches in whole 256-row m-tiles (clipx_encode.hip: ragged_prepare, by the planner of clipx_ragged_plan.h).

Where the folded GEMMs of a ragged text batch run in the 256x256 kernel, its row count is rounded up to a multiple of 256 with
duplicates of real rows (pseudo-samples that are prefixes of the longest caption), so that no GEMM needs a second launch for a
handful of leftover rows.  The pad rows are never read: every embedding must stay the BYTES of the rectangular tower
(OPT_RAGGED_TEXT = 0), fp16 and f32, and the fp16 range flag must stay clear.  ViT-B/32 text tower (width 512, ctx 77), random
weights.

Which batches are padded: launch_gemm sends an [M, 3 * width] GEMM to the 256x256 kernel when bulk * (3 * width / 256) >=
n_cu / 2, where bulk is the number of m-tiles left after it peeled at most 8 of them.  The batches here are sized from that rule
and the CU count of the device: "large" ones have 8 m-tiles more than the rule needs (padded whatever is peeled), the small
one has fewer than 256 rows (never padded)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T, WIDTH = 77, 512


@pytest.fixture(scope="module")
def enc():
    from clip_retrieval_amd.encoder import get_encoder

    e = get_encoder("random:ViT-B/32")
    assert e.arch.ctx_len == T and e.arch.t_width == WIDTH
    yield e
    e.set_option(e.OPT_RAGGED_TEXT, 1)


def _large_rows():
    """Rows from which a ragged batch is padded for certain on this device (module docstring)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nt = 3 * WIDTH // 256
    return (-(-(n_cu // 2) // nt) + 8) * 256


def _ids(lengths, vocab, seed):
    """Captions of the given lengths: EOT (the highest id) at position length - 1, zeros after it."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((len(lengths), T), dtype=np.int32)
    for b, n in enumerate(lengths):
        ids[b, :n - 1] = rng.integers(1, vocab - 2, n - 1)
        ids[b, n - 1] = vocab - 1
    return ids


def _mixed_lengths(residue, seed):
    """Mixed caption lengths (1 .. 77, both extremes present) whose sum is >= _large_rows() and = residue (mod 256)."""
    rng = np.random.default_rng(seed)
    lens = [1, T] + [int(v) for v in rng.integers(1, T + 1, 244)]
    while sum(lens) + 4 * T < _large_rows() + 256:
        lens.append(T)
    need = (residue - sum(lens)) % 256
    need += 256 if need < 4 else 0          # four more captions of need / 4 rows each: 1 .. 65 rows
    lens += [need // 4 + (1 if i < need % 4 else 0) for i in range(4)]
    assert sum(lens) % 256 == residue and sum(lens) >= _large_rows() and all(1 <= n <= T for n in lens)
    return lens


def _encode(enc, ids, ragged):
    """(fp16 bits, f32 bits, rows the layers ran on) through the device entry point with host ids; checks the range flag."""
    enc.set_option(enc.OPT_RAGGED_TEXT, 1 if ragged else 0)
    B = ids.shape[0]
    assert B <= enc.max_batch
    dev = torch.from_numpy(ids).cuda()
    o16 = torch.zeros(B, enc.embed_dim, dtype=torch.float16, device="cuda")
    o32 = torch.zeros(B, enc.embed_dim, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    enc.encode_text_device(dev.data_ptr(), B, o16.data_ptr(), o32.data_ptr(), st, ids_host=ids)
    enc.check_range(st)
    return o16.cpu().numpy().view(np.uint16), o32.cpu().numpy().view(np.uint32), enc.last_text_rows()


def _check(enc, lengths, seed, padded, other=None):
    ids = _ids(lengths, enc.arch.vocab, seed)
    M = int(sum(lengths))
    want16, want32, rows = _encode(enc, ids, ragged=False)
    assert rows == len(lengths) * T
    got16, got32, rows = _encode(other or enc, ids, ragged=True)
    assert rows == ((M + 255) // 256 * 256 if padded else M), (rows, M)
    assert np.isfinite(got32.view(np.float32)).all()
    assert np.array_equal(got16, want16), "fp16 embeddings differ from the rectangular tower"
    assert np.array_equal(got32, want32), "f32 embeddings differ from the rectangular tower"
    return ids, got16, got32


@pytest.mark.parametrize("residue", [1, 255])
def test_leftover_rows_are_padded_to_whole_tiles(enc, residue):
    """One leftover row and 255 leftover rows: 255 pad rows / one pad row."""
    lengths = _mixed_lengths(residue, seed=10 + residue)
    assert len(lengths) <= enc.max_batch
    _check(enc, lengths, seed=20 + residue, padded=True)


def test_whole_tiles_already(enc):
    """A row count that is a multiple of 256: nothing is appended."""
    lengths = _mixed_lengths(0, seed=3)
    _check(enc, lengths, seed=4, padded=False)


def test_small_batch_is_not_padded(enc):
    """Below the threshold every row runs in one 128x128 launch anyway: nothing is appended, same bytes."""
    lengths = [3, 1, 17, 9, 25, 2, 30, 11, 5]
    assert sum(lengths) < 256
    _check(enc, lengths, seed=5, padded=False)


def test_full_length_captions_pad_past_the_rectangular_rows():
    """Every caption at full length, the batch as large as the workspace allows, B * 77 not a multiple of 256: the pad rows lie
    past row max_batch * 77 of every activation buffer (the buffer-size case)."""
    from clip_retrieval_amd.encoder import ARCHS, ClipEncoder, get_encoder, random_blob

    B = -(-_large_rows() // T)
    while (B * T) % 256 == 0:
        B += 1
    arch = ARCHS["ViT-B/32"]
    os.environ["CLIPX_MAX_BATCH"] = str(B)
    try:
        small = ClipEncoder(arch, random_blob(arch, 0), 0)  # the weights of get_encoder("random:ViT-B/32")
    finally:
        os.environ.pop("CLIPX_MAX_BATCH")
    try:
        assert small.max_batch == B
        ref = get_encoder("random:ViT-B/32")
        try:
            _check(ref, [T] * B, seed=6, padded=True, other=small)
        finally:
            ref.set_option(ref.OPT_RAGGED_TEXT, 1)
    finally:
        small.close()


def test_pad_longer_than_the_longest_caption(enc):
    """Equally short captions and one leftover row: the 255 pad rows need several pseudo-samples (at least ceil(255 / 77) = 4, the
    last one shortened).  The captions are the shortest with which max_batch of them reach the padding threshold."""
    lengths = None
    for lmax in range(1, T + 1):
        for n in range(-(-_large_rows() // lmax), enc.max_batch):
            last = (1 - n * lmax) % 256
            if 1 <= last <= lmax:
                lengths = [lmax] * n + [last]
                break
        if lengths:
            break
    assert lengths and sum(lengths) % 256 == 1 and sum(lengths) >= _large_rows()
    _check(enc, lengths, seed=7, padded=True)


def test_caption_order_does_not_change_a_caption(enc):
    """The same captions in another order (another longest-caption index, other pad rows): the same rows per caption."""
    lengths = _mixed_lengths(1, seed=8)
    ids, got16, got32 = _check(enc, lengths, seed=9, padded=True)
    perm = np.random.default_rng(0).permutation(len(lengths))
    p16, p32, rows = _encode(enc, np.ascontiguousarray(ids[perm]), ragged=True)
    assert rows % 256 == 0
    assert np.array_equal(p16, got16[perm]) and np.array_equal(p32, got32[perm])
