"""The Huffman stage of the JPEG decoder on the GPU (csrc/jpeg_huff_kernels.hip, clipx_jpeg_entropy_device): its records
against the host entropy stage's byte for byte, its pixels against Pillow's, not a byte outside records and statuses, malformed files
refused exactly where the host stage defers, and the reader / worker end to end with the late Pillow branch."""
import io
import json
import os
import tarfile

import numpy as np
import pytest

import jpeg_inputs as J
from test_jpeg_huffman_cpu import mutants
from test_service_gpu import tiny_checkpoints  # noqa: F401  (the tiny model's checkpoints, a module-scoped fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
STATUS_SENTINEL = 0x5A5A5A5A


def _entropy_batch(lib, files, gap=48, stream=None, split_bytes=0):
    """files: [jpeg bytes] that pass the host preparation -> ONE clipx_jpeg_entropy_device call (split_bytes > 0: one
    clipx_jpeg_entropy_split_device call with that cut).  The output records lie `gap` bytes
    (a multiple of 16) apart in a buffer pre-filled with a sentinel, the status array has sentinel words behind it; collect() returns
    (statuses, [record bytes], descs, device coefficient buffer) after checking that every byte outside them still holds it."""
    import torch

    from clip_retrieval_amd import jpeg

    packed = [jpeg.scan_packed(d, lib=lib) for d in files]
    assert all(p is not None for p in packed)
    scans, descs, offs, _ = jpeg.pack_scans(packed)
    n = len(files)
    sizes = np.asarray([jpeg.record_bytes(d) for d in descs], dtype=np.int64)
    starts = gap + np.concatenate([[0], np.cumsum(((sizes + 15) & ~15) + gap)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    descs["coef_off"] = starts
    total = int(starts[-1] + sizes[-1] + gap) if n else gap
    coefs = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 3,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the sentinel fills ran on the current stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        dev = scans.cuda() if n else torch.zeros(16, dtype=torch.uint8, device="cuda")
        jpeg.entropy_device(0, dev, descs, offs, coefs, status, stream.cuda_stream if stream is not None else None, lib, split_bytes=split_bytes)

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
        assert dev.numel() >= 16  # (keeps the device copy of the scans alive until the kernel is done)
        return st[:n], records, descs, coefs

    return collect


def _assert_records_equal_host(lib, files, statuses, records, names=None):
    from clip_retrieval_amd import jpeg

    for i, (data, st, rec) in enumerate(zip(files, statuses, records)):
        name = names[i] if names else i
        want = jpeg.entropy(data, lib=lib)
        assert want is not None and st == 0, f"{name}: status {st}"
        bad = int((rec != want[1]).sum())
        assert rec.size == want[1].size and bad == 0, f"{name}: {bad} of {rec.size} record bytes differ from the host stage's"


@pytest.mark.parametrize("part", range(4))
def test_records_equal_the_host_stage(lib, part):
    """The whole input set of test_jpeg_cpu.py in the four batches test_jpeg_gpu.py uses: sides 1 .. 250, one-MCU images, partial MCUs,
    all four samplings, restart intervals 1 and 3 (the RSTn count wraps), optimised tables, long codes, heavy FF 00 stuffing."""
    items = J.cases()[part::4]
    statuses, records, _, _ = _entropy_batch(lib, [d for _, d in items])()
    _assert_records_equal_host(lib, [d for _, d in items], statuses, records, [n for n, _ in items])


def _pixels_after(lib, items, collect, stream=None):
    """The pixel stage behind a collected Huffman launch, on the same stream -> list of uint8 [h, w, 3]."""
    import torch

    from clip_retrieval_amd import jpeg

    statuses, _, descs, coefs = collect()
    assert (statuses == 0).all()
    nbytes = descs["height"].astype(np.int64) * descs["width"] * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        pix = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device="cuda")
        jpeg.pixels_device(0, coefs, descs, pix, offsets, stream.cuda_stream if stream is not None else None, lib)
    (stream or torch.cuda.current_stream()).synchronize()
    flat = pix.cpu().numpy()
    return [flat[o:o + n].reshape(int(d["height"]), int(d["width"]), 3) for d, o, n in zip(descs, offsets, nbytes)]


def _assert_equal_pillow(items, got):
    want = J.pillow_rgb()
    for (name, _), px in zip(items, got):
        assert px.shape == want[name].shape, name
        bad = int((px != want[name]).sum())
        assert bad == 0, f"{name}: {bad} of {px.size} bytes differ from Pillow's"


@pytest.mark.parametrize("part", range(2))
def test_huffman_then_pixel_stage_equals_pillow(lib, part):
    """Huffman kernel, then the pixel stage on the same stream, reading the records where the kernel left them."""
    items = J.cases()[part::2]
    _assert_equal_pillow(items, _pixels_after(lib, items, _entropy_batch(lib, [d for _, d in items])))


def _raw_batch(arrays):
    from clip_retrieval_amd.reader import _collate

    return _collate([{"image_raw": a, "image_filename": str(i)} for i, a in enumerate(arrays)], True, False, False, True)["image_raw"]


def test_scan_batch_feeds_the_gpu_resize(lib):
    """Scans through `_collate` and encoder.resize_crop_device: Huffman, pixel stage and resize on the GPU; the crops equal those
    from Pillow-decoded pixels, S = 224; no row is dropped."""
    import torch
    from PIL import Image

    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.encoder import resize_crop_device

    files = []
    for name in J.BASELINE_GOLDENS:
        with open(os.path.join(J.GOLDEN, "test_images", name), "rb") as f:
            files.append(f.read())
    files.append(J.encode(J.content("noise", 256, 256, 11), 2, 95, False, 0))
    huff = R.DecodeRgbU8(224, gpu_huffman=True)
    samples = [R._decode_sample({"key": str(i), "image": d, "text": None, "metadata": None}, huff, None, True, False, False) for i, d in enumerate(files)]
    assert all("image_jpeg_scan" in s for s in samples)
    batch = R._collate(samples, True, False, False, True)
    got = resize_crop_device(lib, 0, 224, batch["image_raw"], None, batch["image_jpeg_scan"])
    want = resize_crop_device(lib, 0, 224, _raw_batch([np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in files]))
    torch.cuda.synchronize()
    assert got._clipx_kept is None and got.shape == (3, 224, 224, 3) and torch.equal(got, want)


def test_batch_shapes(lib):
    cases = J.cases()
    pick = [c for c in cases if c[0].startswith("131x250-s2")][:1] + [c for c in cases if c[0].startswith("33x15-s1")][:1] + \
        [c for c in cases if c[0].startswith("16x33-sL")][:1]
    assert len(pick) == 3
    # B = 0: a no-op that writes nothing
    statuses, records, _, _ = _entropy_batch(lib, [])()
    assert statuses.size == 0 and records == []
    for b in (1, 2, 3):
        files = [d for _, d in pick[:b]]
        statuses, records, _, _ = _entropy_batch(lib, files, gap=16)()
        _assert_records_equal_host(lib, files, statuses, records)
    # a whole part in reversed order: the largest image last, the records elsewhere
    items = cases[1::4][::-1]
    statuses, records, _, _ = _entropy_batch(lib, [d for _, d in items], gap=32)()
    _assert_records_equal_host(lib, [d for _, d in items], statuses, records, [n for n, _ in items])


def test_two_streams_decode_at_once(lib):
    """Different batches on two streams, launches interleaved and more of them than the table ring has slots: all exact, and the
    pixel stage behind each on its stream gives Pillow's bytes."""
    import torch

    cases = J.cases()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = []
    for k in range(6):
        items = cases[k::6]
        pending.append((items, streams[k % 2], _entropy_batch(lib, [d for _, d in items], gap=80, stream=streams[k % 2])))
    for items, stream, collect in pending:
        _assert_equal_pillow(items, _pixels_after(lib, items, collect, stream))


@pytest.mark.parametrize("split_bytes", [0, 128])
def test_table_regrowth_across_ring_wraps(lib, split_bytes):
    """B = 1 and B = 768 images of 8 x 8 in turn, nine calls, through clipx_jpeg_entropy_device and through the split entry at 128
    bytes: the ring of four table slots wraps twice, and a slot that held the 64 KiB floor meets a table of 768 x 88 bytes = 66 KiB and
    grows.  All launched before the first is collected; every status 0, every record the host stage's, no byte outside them written
    (checked in collect())."""
    files = [J.encode(J.content(J.CONTENTS[i % 3], 8, 8, 300 + i), J.SAMPLINGS[i % 4], J.QUALITIES[(i // 4) % 4], False, 0) for i in range(768)]
    calls = [files[:1] if k % 2 == 0 else files for k in range(9)]
    pending = [_entropy_batch(lib, batch, gap=16, split_bytes=split_bytes) for batch in calls]
    for k, (batch, collect) in enumerate(zip(calls, pending)):
        statuses, records, _, _ = collect()
        assert statuses.shape == (len(batch),) and (statuses == 0).all(), f"call {k}: statuses {np.unique(statuses)}"
        _assert_records_equal_host(lib, batch, statuses, records, [f"call {k}, image {i}" for i in range(len(batch))])


@pytest.fixture(scope="module")
def malformed(lib):
    """The first 600 mutants of the seed-7 sequence in ONE launch -> (files that passed the host preparation, their statuses, their
    records, whether the host entropy stage takes each).  Input validation of a kernel whose loops are bounded and whose every
    access ran under the sanitizers on the CPU first (test_jpeg_huffman_cpu.py)."""
    from clip_retrieval_amd import jpeg

    files = [m for m in mutants(600) if jpeg.scan_packed(m, lib=lib) is not None]
    statuses, records, _, _ = _entropy_batch(lib, files)()  # (sentinels between and behind the records and the statuses: checked inside)
    host = [jpeg.entropy(m, lib=lib) for m in files]
    return files, statuses, records, host


def test_malformed_files_are_refused_exactly_where_the_host_stage_defers(malformed):
    files, statuses, records, host = malformed
    clean = unclean = 0
    for i, (st, rec, want) in enumerate(zip(statuses, records, host)):
        assert (st == 0) == (want is not None), f"mutant {i}: status {st}, host stage {'takes' if want is not None else 'defers'}"
        assert 0 <= st <= 7
        if want is not None:
            assert np.array_equal(rec, want[1]), f"mutant {i}: the record differs from the host stage's"
            clean += 1
        else:
            unclean += 1
    print(f"{len(files)} of 600 mutants reach the kernel: {unclean} unclean, {clean} clean")
    assert len(files) >= 400 and unclean >= 80 and clean >= 300


def _late_kinds(malformed):
    """(a mutant the kernel refuses and Pillow still decodes, one on which Pillow raises too)."""
    from PIL import Image, UnidentifiedImageError

    from clip_retrieval_amd.reader import DecodeRgbU8

    files, statuses, _, _ = malformed
    decodes = raises = None
    for data, st in zip(files, statuses):
        if st == 0:
            continue
        try:
            px = np.asarray(DecodeRgbU8(224)(Image.open(io.BytesIO(data))))
            if decodes is None and px.ndim == 3:
                decodes = data
        except (UnidentifiedImageError, OSError, ValueError):
            if raises is None:
                raises = data
    assert decodes is not None and raises is not None, "the refused mutants hold no file of each kind"
    return decodes, raises


def _golden(name):
    with open(os.path.join(J.GOLDEN, "test_images", name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def late_tar(malformed, tmp_path_factory):
    """A shard with the two baseline goldens, a progressive golden, a PNG, a truncated JPEG and one refused mutant of each kind, each
    with a caption -> (path, member keys in order, keys no setting may let through)."""
    from PIL import Image

    decodes, raises = _late_kinds(malformed)
    png = io.BytesIO()
    Image.fromarray(J.content("gradient", 40, 24, 1)).save(png, "PNG")
    base = _golden(J.BASELINE_GOLDENS[0])
    members = [("base0", base), ("raises", raises), ("prog", _golden(J.PROGRESSIVE_GOLDENS[0])), ("png", png.getvalue()),
               ("truncated", base[:len(base) // 2]), ("decodes", decodes), ("base1", _golden(J.BASELINE_GOLDENS[1]))]
    path = str(tmp_path_factory.mktemp("late") / "late.tar")
    with tarfile.open(path, "w") as tf:
        for key, data in members:
            for ext, blob in (("jpg", data), ("txt", f"a photo of {key}".encode())):
                ti = tarfile.TarInfo(f"{key}.{ext}")
                ti.size = len(blob)
                tf.addfile(ti, io.BytesIO(blob))
    return path, [k for k, _ in members], ("raises", "truncated")


SETTINGS = ({"gpu_huffman": True}, {"gpu_jpeg": True}, {})


def test_reader_and_resize_with_the_late_branch(lib, late_tar):
    """The reader and resize_crop_device over that shard with gpu_huffman on, gpu_jpeg alone and both off: the crops are byte-equal
    row for row; the mutant Pillow refuses and the truncated file are absent from all three; with gpu_huffman on both mutants did
    reach the kernel, one came back through Pillow and one was dropped."""
    import torch

    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.encoder import resize_crop_device
    from clip_retrieval_amd.runner import Sampler

    path, keys, absent = late_tar

    def run(**switches):
        r = R.WebdatasetReader(Sampler(0, 1), R.DecodeRgbU8(224, **switches), None, [path], 3, 2, enable_text=False)
        r.use_processes = False
        crops, names, scanned, dropped = [], [], 0, 0
        for b in r:
            assert ("image_jpeg_scan" in b) <= bool(switches.get("gpu_huffman")) and ("image_jpeg" in b) <= (switches == {"gpu_jpeg": True})
            jp = b.get("image_jpeg_scan") or b.get("image_jpeg")
            out = resize_crop_device(lib, 0, 224, b["image_raw"], None, jp)
            kept = out._clipx_kept
            scanned += len(b["image_jpeg_scan"]["slots"]) if "image_jpeg_scan" in b else 0
            dropped += 0 if kept is None else len(b["image_filename"]) - len(kept)
            names += b["image_filename"] if kept is None else [b["image_filename"][i] for i in kept]
            crops.append(out.cpu())
        return torch.cat(crops), names, scanned, dropped

    results = [run(**s) for s in SETTINGS]
    want_names = [k for k in keys if k not in absent]
    for crops, names, scanned, dropped in results:
        assert names == want_names and crops.shape == (len(want_names), 224, 224, 3)
        assert torch.equal(crops, results[-1][0])
    assert results[0][2:] == (4, 1) and results[1][2:] == (0, 0) and results[2][2:] == (0, 0)  # base0, raises, decodes, base1 travelled as scans


def test_worker_with_the_late_branch_and_the_default(tiny_checkpoints, late_tar, tmp_path):  # noqa: F811
    """worker() with the tiny model over that shard: embeddings, filenames and captions written are equal file for file across the
    three settings, `sample_count` is the number of rows written, and worker() without the new argument is the gpu_jpeg path."""
    import inspect

    import pandas as pd

    from clip_retrieval_amd import reader as R
    from clip_retrieval_amd.runner import Sampler
    from clip_retrieval_amd.worker import worker

    _, _, dirs = tiny_checkpoints
    path, keys, absent = late_tar
    rows = len(keys) - len(absent)
    outs = []
    for i, switches in enumerate(SETTINGS):
        out = tmp_path / f"out{i}"
        worker(tasks=[0], input_dataset=[path], output_folder=str(out), output_partition_count=1, input_format="webdataset", batch_size=3,
               num_prepro_workers=2, enable_text=True, enable_image=True, enable_metadata=False, clip_model="tiny-test",
               clip_cache_path=dirs["openai"], device=0, gpu_resize=True, **switches)
        img, txt = np.load(out / "img_emb" / "img_emb_0.npy"), np.load(out / "text_emb" / "text_emb_0.npy")
        meta = pd.read_parquet(out / "metadata" / "metadata_0.parquet")
        assert img.shape[0] == txt.shape[0] == len(meta) == rows
        assert json.loads((out / "stats" / "0.json").read_text())["sample_count"] == rows
        outs.append((img, txt, meta))
    for img, txt, meta in outs[:-1]:
        assert np.array_equal(img, outs[-1][0]) and np.array_equal(txt, outs[-1][1]) and meta.equals(outs[-1][2])
    assert list(outs[0][2]["image_path"]) == [k for k in keys if k not in absent]
    assert list(outs[0][2]["caption"]) == [f"a photo of {k}" for k in keys if k not in absent]

    # the default: the argument exists, is off, and a reader built without it yields the gpu_jpeg path's batches, key for key and byte for byte
    assert inspect.signature(worker).parameters["gpu_huffman"].default is False

    def batches(pre):
        r = R.WebdatasetReader(Sampler(0, 1), pre, None, [path], 3, 2, enable_text=False)
        r.use_processes = False
        return list(r)

    for a, b in zip(batches(R.DecodeRgbU8(224, gpu_jpeg=True)), batches(R.DecodeRgbU8(224, gpu_jpeg=True, gpu_huffman=False)), strict=True):
        assert sorted(a) == sorted(b) and "image_jpeg_scan" not in a and a["image_filename"] == b["image_filename"]
        assert all(np.array_equal(a["image_raw"][k], b["image_raw"][k]) for k in ("offsets", "hw")) and a["image_raw"]["pixels"].numel() == b["image_raw"]["pixels"].numel()
        reserved = a["image_jpeg"]["slots"].tolist() if "image_jpeg" in a else []
        for row, (o, (h, w)) in enumerate(zip(a["image_raw"]["offsets"], a["image_raw"]["hw"])):
            if row not in reserved:  # (a reserved slot is left unwritten on the host)
                assert np.array_equal(a["image_raw"]["pixels"].numpy()[o:o + h * w * 3], b["image_raw"]["pixels"].numpy()[o:o + h * w * 3])
        if "image_jpeg" in a:
            assert sorted(a["image_jpeg"]) == sorted(b["image_jpeg"]) == ["coefs", "descs", "slots"]
            assert np.array_equal(a["image_jpeg"]["coefs"].numpy(), b["image_jpeg"]["coefs"].numpy())
            assert a["image_jpeg"]["descs"].tobytes() == b["image_jpeg"]["descs"].tobytes() and a["image_jpeg"]["slots"].tolist() == b["image_jpeg"]["slots"].tolist()
