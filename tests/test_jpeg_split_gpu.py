"""The split Huffman decode inside a restart interval on the GPU (csrc/jpeg_split_kernels.hip, clipx_jpeg_entropy_split_device; DESIGN
9.2): records against the host entropy stage's byte for byte, the rounds word against the host form of the same decoder, not a byte
outside records, statuses and rounds, malformed files refused with the serial kernel's codes, and the reader end to end."""
import numpy as np
import pytest

import jpeg_inputs as J
import jpeg_split_inputs as SI
from test_jpeg_huffman_cpu import mutants
from test_jpeg_huffman_gpu import (SENTINEL, STATUS_SENTINEL, _assert_equal_pillow, _assert_records_equal_host, _entropy_batch, _pixels_after,
                                   late_tar, malformed)  # noqa: F401  (the last two: module-scoped fixtures)
from test_service_gpu import tiny_checkpoints  # noqa: F401

pytestmark = pytest.mark.gpu


def _split_batch(lib, files, split, max_rounds=0, gap=48, stream=None, want_rounds=True):
    """test_jpeg_huffman_gpu._entropy_batch for ONE clipx_jpeg_entropy_split_device call: the same sentinels around the records and
    behind the statuses, and behind the rounds words too.  collect() -> (statuses, [record bytes], descs, device coefficient buffer,
    rounds)."""
    import torch

    from clip_retrieval_amd import jpeg

    packed = [jpeg.scan_packed(d, lib=lib) for d in files]
    assert all(p is not None for p in packed)
    scans, descs, offs, _ = jpeg.pack_scans(packed)
    n = len(files)
    sizes = np.asarray([jpeg.record_bytes(d) for d in descs], dtype=np.int64)
    starts = gap + np.concatenate([[0], np.cumsum(((sizes + 15) & ~15) + gap)[:-1]]).astype(np.int64)
    descs["coef_off"] = starts
    total = int(starts[-1] + sizes[-1] + gap)
    coefs = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 3,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    rounds = torch.full((n + 3,), STATUS_SENTINEL, dtype=torch.int32, device="cuda") if want_rounds else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        dev = scans.cuda()
        jpeg.entropy_device(0, dev, descs, offs, coefs, status, stream.cuda_stream if stream is not None else None, lib, split_bytes=split,
                            max_rounds=max_rounds, rounds_dev=rounds)

    def collect():
        (stream or torch.cuda.current_stream()).synchronize()
        flat, st = coefs.cpu().numpy(), status.cpu().numpy()
        outside = np.ones(total, dtype=bool)
        records = []
        for o, s in zip(starts, sizes):
            records.append(flat[o:o + s])
            outside[o:o + s] = False
        assert (flat[outside] == SENTINEL).all(), "bytes outside the records were written"
        assert (st[n:] == STATUS_SENTINEL).all(), "words behind the status array were written"
        rd = rounds.cpu().numpy() if want_rounds else None
        assert rd is None or (rd[n:] == STATUS_SENTINEL).all(), "words behind the rounds array were written"
        assert dev.numel() >= 16
        return st[:n], records, descs, coefs, None if rd is None else rd[:n]

    return collect


def _host_rounds(lib, files, split, max_rounds):
    from clip_retrieval_amd import jpeg

    out = []
    for d in files:
        packed = jpeg.scan_packed(d, lib=lib)
        out.append(jpeg.entropy_split_host(packed[64:], packed[:64].view(jpeg.JPEG_DESC), split, max_rounds, lib=lib)[2])
    return np.asarray(out, dtype=np.int32)


def _check(lib, items, split, max_rounds=0, **kw):
    files = [d for _, d in items]
    statuses, records, _, _, rounds = _split_batch(lib, files, split, max_rounds, **kw)()
    _assert_records_equal_host(lib, files, statuses, records, [n for n, _ in items])
    want = _host_rounds(lib, files, split, max_rounds)
    assert np.array_equal(rounds, want), [(n, int(a), int(b)) for (n, _), a, b in zip(items, rounds, want) if a != b]
    return rounds


@pytest.mark.parametrize("split", (32, 128))
@pytest.mark.parametrize("part", range(5))
def test_records_and_rounds_equal_the_host_stage(lib, part, split):
    """The four batches of the 146 files (restart intervals 0 / 1 / 3: split and unsplit intervals in one image, short last
    intervals) and, as part 4, the no-restart-marker set, at max_rounds 4096: nothing falls back, records and rounds are the host's."""
    items = J.cases()[part::4] if part < 4 else SI.cases()
    rounds = _check(lib, items, split, 4096)
    assert (rounds >= 0).all() and (rounds >= 2).any()
    if part == 4:
        assert rounds.max() >= 64  # the stripes: as many rounds as sub-sequences


def test_cap_of_one_round_and_the_default_cap(lib):
    """max_rounds 1: every split interval gives up and is decoded serially by the same workgroup; the default cap: the periodic
    files give up, the others do not; the records are the host stage's either way."""
    rounds = _check(lib, SI.cases(), 128, 1)
    assert set(rounds.tolist()) <= {0, -1} and (rounds == -1).sum() >= 20
    rounds = _check(lib, SI.cases(), 32, 0)
    from clip_retrieval_amd import jpeg

    assert (rounds < 0).any() and (rounds >= 2).any() and rounds.min() == -jpeg.SPLIT_DEFAULT_ROUNDS  # (the default: DESIGN 9.2)


def test_split_then_pixel_stage_equals_pillow(lib):
    import torch  # noqa: F401

    items = SI.cases()
    collect = _split_batch(lib, [d for _, d in items], 128, 4096)
    got = _pixels_after(lib, items, lambda: collect()[:4])
    want = SI.pillow_rgb()
    for (name, _), px in zip(items, got):
        assert px.shape == want[name].shape and np.array_equal(px, want[name]), name


def test_malformed_files_get_the_serial_kernels_codes(lib):
    """The first 300 mutants at split 32 against clipx_jpeg_entropy_device on the same batch: code for code; zero exactly where the
    host stage takes the file, and then its record."""
    from clip_retrieval_amd import jpeg

    files = [m for m in mutants(300) if jpeg.scan_packed(m, lib=lib) is not None]
    serial, _, _, _ = _entropy_batch(lib, files)()
    statuses, records, _, _, rounds = _split_batch(lib, files, 32, 4096)()
    diff = [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(statuses, serial)) if a != b]
    assert not diff, diff[:10]
    unclean = 0
    for i, (m, st, rec) in enumerate(zip(files, statuses, records)):
        want = jpeg.entropy(m, lib=lib)
        assert (st == 0) == (want is not None), i
        if want is not None:
            assert np.array_equal(rec, want[1]), i
        unclean += st != 0
    assert len(files) >= 200 and unclean >= 40 and (rounds >= 2).sum() >= 100
    assert np.array_equal(rounds, _host_rounds(lib, files, 32, 4096))


def test_two_streams_b1_and_a_mixed_batch(lib):
    import torch

    # two streams at once, more launches than the table ring has slots
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cases = J.cases()[::3] + SI.cases()
    pending = []
    for k in range(6):
        items = cases[k::6]
        pending.append((items, _split_batch(lib, [d for _, d in items], (32, 128)[k % 2], 4096, gap=80, stream=streams[k % 2])))
    for items, collect in pending:
        statuses, records, _, _, _ = collect()
        _assert_records_equal_host(lib, [d for _, d in items], statuses, records, [n for n, _ in items])
    # B = 1: a split image, an unsplit one, and no rounds array
    big = [c for c in SI.cases() if c[0].startswith("256x256") and "-photo-" in c[0]][:1]
    small = [c for c in J.cases() if c[0].startswith("3x4-")][:1]
    assert _check(lib, big, 128, 4096, gap=16)[0] >= 2 and _check(lib, small, 128, 4096, gap=16)[0] == 0
    statuses, records, _, _, rounds = _split_batch(lib, [big[0][1]], 256, 0, want_rounds=False)()
    assert rounds is None
    _assert_records_equal_host(lib, [big[0][1]], statuses, records)
    # split and unsplit images alternating: every other image is a gray file so small that its record has no room for an interval
    # of 1 024 bytes -- those go to huff_kernel, and the launches alternate between the kernels
    tiny = [c for c in J.cases() if "-sL-" in c[0] and len(c[1]) < 900][:8]
    assert len(tiny) == 8
    large = [c for c in SI.cases() if len(c[1]) > 8000][:8]
    mixed = [x for pair in zip(tiny, large) for x in pair] + tiny[:3]
    rounds = _check(lib, mixed, 512, 4096, gap=32)
    assert (rounds[1:16:2] >= 2).all() and (rounds[0:16:2] == 0).all() and (rounds[16:] == 0).all()


def test_reader_and_resize_with_the_split_switch(lib, late_tar):  # noqa: F811
    """DecodeRgbU8(gpu_huffman=True, huffman_split=128) through reader + resize over the shard with the late branch: the rows and
    their bytes are those of huffman_split=0."""
    import torch

    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.encoder import resize_crop_device
    from clip_retrieval_amd.runner import Sampler

    path, keys, absent = late_tar

    def run(**switches):
        r = R.WebdatasetReader(Sampler(0, 1), R.DecodeRgbU8(224, **switches), None, [path], 3, 2, enable_text=False)
        r.use_processes = False
        crops, names, seen = [], [], []
        for b in r:
            seen.append(b["image_jpeg_scan"].get("split_bytes") if "image_jpeg_scan" in b else None)
            out = resize_crop_device(lib, 0, 224, b["image_raw"], None, b.get("image_jpeg_scan"))
            kept = out._clipx_kept
            names += b["image_filename"] if kept is None else [b["image_filename"][i] for i in kept]
            crops.append(out.cpu())
        return torch.cat(crops), names, seen

    on, off = run(gpu_huffman=True, huffman_split=128), run(gpu_huffman=True)
    assert on[1] == off[1] == [k for k in keys if k not in absent] and torch.equal(on[0], off[0])
    assert 128 in on[2] and set(on[2]) <= {128, None} and set(off[2]) <= {None}
