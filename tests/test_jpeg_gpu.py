"""The pixel stage of the JPEG decoder on the GPU (csrc/jpeg_kernels.hip, clipx_jpeg_pixels_device) against Pillow: every
byte of every file of the accepted class, not a byte outside the images, the hand-over to the GPU resize, and the reader end to end
with the switch on and off."""
import functools
import io
import os
import tarfile

import numpy as np
import pytest

import jpeg_inputs as J

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def _decode_batch(lib, items, gap=5, stream=None):
    """items: [(name, jpeg bytes)] -> list of uint8 [h, w, 3] from ONE clipx_jpeg_pixels_device call.  The images lie `gap` bytes
    apart (odd: unaligned starts) in a buffer pre-filled with a sentinel; every byte outside them must still hold it afterwards."""
    import torch

    from clip_retrieval_amd import jpeg

    got = [jpeg.entropy_packed(data, lib=lib) for _, data in items]
    assert all(g is not None for g in got), [n for (n, _), g in zip(items, got) if g is None]
    coefs, descs = jpeg.pack_records(got)
    nbytes = descs["height"].astype(np.int64) * descs["width"] * 3
    offsets = np.zeros(len(items), dtype=np.int64)
    offsets[0] = gap
    offsets[1:] = gap + np.cumsum(nbytes[:-1] + gap)
    total = int(offsets[-1] + nbytes[-1] + gap)
    pix = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the sentinel fill ran on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        dev = coefs.cuda()
        jpeg.pixels_device(0, dev, descs, pix, offsets, stream.cuda_stream if stream is not None else None, lib)

    def collect():
        (stream or torch.cuda.current_stream()).synchronize()
        flat = pix.cpu().numpy()
        outside = np.ones(total, dtype=bool)
        out = []
        for d, o, n in zip(descs, offsets, nbytes):
            out.append(flat[o:o + n].reshape(int(d["height"]), int(d["width"]), 3))
            outside[o:o + n] = False
        assert (flat[outside] == SENTINEL).all(), "bytes outside the images were written"
        assert dev.numel() == coefs.numel()  # (keeps the device copy of the coefficients alive until the kernels are done)
        return out

    return collect


def _assert_equal_pillow(items, got):
    want = J.pillow_rgb()
    for (name, _), px in zip(items, got):
        assert px.shape == want[name].shape, name
        bad = int((px != want[name]).sum())
        assert bad == 0, f"{name}: {bad} of {px.size} bytes differ from Pillow's"


@pytest.mark.parametrize("part", range(4))
def test_every_byte_equals_pillow(lib, part):
    """The whole input set of test_jpeg_cpu.py in four batches that mix sizes, samplings, restart intervals and grayscale."""
    items = J.cases()[part::4]
    _assert_equal_pillow(items, _decode_batch(lib, items)())


def test_small_batches(lib):
    cases = J.cases()
    one = [c for c in cases if c[0].startswith("131x250-s2")][:1]
    _assert_equal_pillow(one, _decode_batch(lib, one)())
    dots = [c for c in cases if c[0].startswith("1x1-")]  # every sampling and content at 1 x 1
    assert len(dots) == 12
    _assert_equal_pillow(dots, _decode_batch(lib, dots, gap=1)())
    # B = 64 images of 8 x 8 in one launch
    from PIL import Image

    many, want = [], []
    for i in range(64):
        data = J.encode(J.content(J.CONTENTS[i % 3], 8, 8, 100 + i), J.SAMPLINGS[i % 4], J.QUALITIES[(i // 4) % 4], False, 0)
        many.append((f"8x8-{i}", data))
        want.append(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    for w, g in zip(want, _decode_batch(lib, many, gap=3)()):
        assert np.array_equal(w, g)


def _raw_batch(arrays):
    from clip_retrieval_amd.reader import _collate

    return _collate([{"image_raw": a, "image_filename": str(i)} for i, a in enumerate(arrays)], True, False, False, True)["image_raw"]


def test_output_feeds_the_gpu_resize(lib):
    """Decoded on the GPU into the image_raw layout and resized there: the crops equal those from Pillow-decoded pixels, S = 224."""
    import torch
    from PIL import Image

    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.encoder import resize_crop_device

    files = []
    for name in J.BASELINE_GOLDENS:
        with open(os.path.join(J.GOLDEN, "test_images", name), "rb") as f:
            files.append(f.read())
    files.append(J.encode(J.content("noise", 256, 256, 11), 2, 95, False, 0))
    on = R.DecodeRgbU8(224, gpu_jpeg=True)
    samples = [R._decode_sample({"key": str(i), "image": d, "text": None, "metadata": None}, on, None, True, False, False) for i, d in enumerate(files)]
    assert all("image_jpeg" in s for s in samples)
    batch = R._collate(samples, True, False, False, True)
    got = resize_crop_device(lib, 0, 224, batch["image_raw"], None, batch["image_jpeg"])
    want = resize_crop_device(lib, 0, 224, _raw_batch([np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in files]))
    torch.cuda.synchronize()
    assert got.shape == (3, 224, 224, 3) and torch.equal(got, want)


def test_reader_end_to_end_switch_on_and_off(lib):
    """The reader over the reference's tar shards: identical [B, S, S, 3] crops for the encoder with the switch on and off; the
    baseline members took the GPU path, the progressive ones went through Pillow."""
    import torch
    from PIL import Image

    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.encoder import resize_crop_device
    from clip_retrieval_amd.runner import Sampler

    tars = [os.path.join(J.GOLDEN, "test_tars", f"image{i}.tar") for i in range(1, 5)]
    baseline = members = 0
    for t in tars:
        with tarfile.open(t) as tf:
            for m in tf:
                if m.isfile() and m.name.endswith(".jpg"):
                    members += 1
                    baseline += not Image.open(io.BytesIO(tf.extractfile(m).read())).info.get("progressive")
    assert 0 < baseline < members

    def run(gpu_jpeg):
        r = R.WebdatasetReader(Sampler(0, 1), R.DecodeRgbU8(224, gpu_jpeg=gpu_jpeg), None, tars, 4, 2, enable_text=False)
        r.use_processes = False  # (the transport through the decode processes: test_jpeg_cpu.py)
        crops, names, taken = [], [], 0
        for b in r:
            jp = b.get("image_jpeg")
            assert (jp is not None) == (gpu_jpeg and any(n in ("123_456", "456_123") for n in b["image_filename"]))
            taken += 0 if jp is None else len(jp["slots"])
            crops.append(resize_crop_device(lib, 0, 224, b["image_raw"], None, jp).cpu())
            names += b["image_filename"]
        return torch.cat(crops), names, taken

    off, names_off, taken_off = run(False)
    on, names_on, taken_on = run(True)
    assert names_on == names_off and len(names_on) == members and on.shape == (members, 224, 224, 3)
    assert taken_off == 0 and taken_on == baseline
    assert torch.equal(on, off)


def test_two_streams_decode_at_once(lib):
    """Different batches on two streams, launches interleaved and more of them than the table ring has slots: all exact."""
    import torch

    cases = J.cases()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = []
    for k in range(6):
        items = cases[k::6]
        pending.append((items, _decode_batch(lib, items, gap=7, stream=streams[k % 2])))
    for items, collect in pending:
        _assert_equal_pillow(items, collect())


@functools.lru_cache(maxsize=None)
def _ring_calls():
    """The calls of the two tests below, built once: B = 1 and B = 768 images of 8 x 8 in turn, nine calls, so that the ring of four
    table slots wraps twice and a slot that held the 64 KiB floor meets a table of 768 x 88 bytes = 66 KiB and grows; then one
    2048 x 2048 4:4:4 image, whose planes (256 x 256 blocks x 3 components x 64 bytes = 12.6 MB) pass the 8 MiB floor of the plane
    scratch; then the B = 1 call again.  -> [(items, Pillow's RGB of each)]"""
    from PIL import Image

    def want(items):
        return [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for _, d in items]

    tiny = [(f"8x8-{i}", J.encode(J.content(J.CONTENTS[i % 3], 8, 8, 300 + i), J.SAMPLINGS[i % 4], J.QUALITIES[(i // 4) % 4], False, 0))
            for i in range(768)]
    one, many = (tiny[:1], want(tiny[:1])), (tiny, want(tiny))
    big = [("2048x2048-s0", J.encode(J.content("gradient", 2048, 2048, 1), 0, 90, False, 0))]
    return [one if k % 2 == 0 else many for k in range(9)] + [(big, want(big)), one]


def _run_ring_calls(lib, streams):
    calls = _ring_calls()
    assert [len(items) for items, _ in calls] == [1, 768, 1, 768, 1, 768, 1, 768, 1, 1, 1]
    pending = [_decode_batch(lib, items, gap=3, stream=streams[k % len(streams)]) for k, (items, _) in enumerate(calls)]
    for k, ((items, want), collect) in enumerate(zip(calls, pending)):
        got = collect()  # (the sentinel bytes around the images: checked inside)
        assert len(got) == len(want)
        for (name, _), w, g in zip(items, want, got):
            assert g.shape == w.shape and np.array_equal(g, w), f"call {k}, {name}: differs from Pillow's decode"


def test_table_and_plane_regrowth_across_ring_wraps(lib):
    """Eleven calls in a row on one stream (see _ring_calls): every image equals Pillow's decode, nothing outside them is written."""
    _run_ring_calls(lib, [None])


def test_table_and_plane_regrowth_on_two_streams(lib):
    """The same calls dealt to two streams in turn, all launched before the first is collected."""
    import torch

    _run_ring_calls(lib, [torch.cuda.Stream(), torch.cuda.Stream()])
