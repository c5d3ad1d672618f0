"""GPU JPEG decode measured against the Pillow decode it replaces, all legs in one process run:

  1. reader rate     images/s of WebdatasetReader with the decode processes running Pillow (DecodeRgbU8) against the same reader
                     with gpu_jpeg=True (entropy stage in the decode processes) + the pixel stage on the GPU for every batch; one
                     core's rate of the entropy stage against Pillow's whole decode beside it;
  2. pixel stage     clipx_jpeg_pixels_device alone on one 256-image batch: time per batch and achieved bytes/s (coefficients
                     read + planes written and read back + RGB written);
  3. pipeline        worker() samples/s from JPEG tar members, image tower only, random weights, gpu_resize with the switch off
                     against on, for ViT-B/32 and ViT-L/14.
Legs 1 and 3 run off / on alternating, several passes each after an untimed pass of both, and print every pass and the medians.

With --legs huffman (or all), the Huffman stage on the device (`gpu_huffman`) beside the two:
  4. Huffman stage   clipx_jpeg_entropy_device alone on a 256-image batch, events around the launch, for files without restart
                     markers (one wave per image) and with one interval per MCU row; the single-core host entropy rate of the
                     same files beside it; the bytes that travel in each form; for the files without restart markers also the
                     split decode inside an interval at 128 / 256 / 512 bytes, alternating with the serial form in
                     the same run, and the distribution of `rounds` over the files;
  5. reader rate     leg 1 with 4 and 16 decode processes, off / host entropy / device entropy / device split 128 / 256 / 512
                     alternating;
  6. pipeline        leg 3 in the same six settings.

The workload: 256 x 256, quality 95, 4:2:0 JPEGs of the project's synthetic images (synth.synth_pixels_u8).  The "off" leg of the
same run is the yardstick.

    python tools/jpeg_bench.py [--workers 16] [--samples 32768] [--rounds 3] [--models ViT-B/32,ViT-L/14] [--legs jpeg|huffman|all]
"""
import argparse
import glob
import io
import os
import shutil
import sys
import tarfile
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_shards(tmp, shards, per):
    from PIL import Image

    from clip_retrieval_amd.synth import synth_pixels_u8

    jpegs = []
    for im in synth_pixels_u8(64, 256):
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="JPEG", quality=95, subsampling=2)
        jpegs.append(buf.getvalue())
    paths = []
    for sh in range(shards):
        path = os.path.join(tmp, f"{sh:03d}.tar")
        with tarfile.open(path, "w") as tf:
            for i in range(per):
                data = jpegs[(sh * per + i) % 64]
                ti = tarfile.TarInfo(f"{sh:03d}{i:06d}.jpg")
                ti.size = len(data)
                tf.addfile(ti, io.BytesIO(data))
        paths.append(path)
    print(f"workload: {shards} shards x {per} JPEGs 256 x 256 q95 4:2:0, mean {np.mean([len(j) for j in jpegs]) / 1024:.1f} KiB", flush=True)
    return paths, jpegs


def reader_rate(paths, workers, gpu_jpeg):
    """One pass of the reader over all shards; every batch is uploaded, (decoded,) and resized on the GPU as the mapper would."""
    import torch

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd.encoder import resize_crop_device
    from clip_retrieval_amd.reader import DecodeRgbU8, WebdatasetReader
    from clip_retrieval_amd.runner import Sampler

    lib = load_library()
    r = WebdatasetReader(Sampler(0, 1), DecodeRgbU8(224, gpu_jpeg=gpu_jpeg), None, paths, 256, workers, enable_text=False)
    t0 = time.perf_counter()
    n = taken = 0
    for b in r:
        jp = b.get("image_jpeg")
        resize_crop_device(lib, 0, 224, b["image_raw"], None, jp)
        n += b["image_raw"]["hw"].shape[0]
        taken += 0 if jp is None else len(jp["slots"])
    torch.cuda.synchronize()
    assert taken == (n if gpu_jpeg else 0)
    return n / (time.perf_counter() - t0)


def entropy_rate(jpegs):
    """One core: the entropy stage against Pillow's whole decode, what bounds the decode processes."""
    from PIL import Image

    from clip_retrieval_amd import jpeg

    t0 = time.perf_counter()
    for j in jpegs * 4:
        jpeg.entropy(j)
    t1 = time.perf_counter()
    for j in jpegs * 4:
        np.asarray(Image.open(io.BytesIO(j)).convert("RGB"))
    t2 = time.perf_counter()
    n = 4 * len(jpegs)
    print(f"one core: entropy stage {n / (t1 - t0):.0f} images/s, Pillow decode {n / (t2 - t1):.0f} images/s", flush=True)


def pixel_stage(jpegs):
    import torch

    from clip_retrieval_amd import jpeg

    coefs, descs = jpeg.pack_records([jpeg.entropy_packed(jpegs[i % 64]) for i in range(256)], True)
    nbytes = descs["height"].astype(np.int64) * descs["width"] * 3
    offsets = np.zeros(256, np.int64)
    np.cumsum(nbytes[:-1], out=offsets[1:])
    dev = coefs.cuda()
    pix = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device="cuda")
    for _ in range(10):
        jpeg.pixels_device(0, dev, descs, pix, offsets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        jpeg.pixels_device(0, dev, descs, pix, offsets)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    planes = int(descs["blocks"].sum()) * 64
    moved = coefs.numel() + 2 * planes + int(nbytes.sum())
    print(f"pixel stage alone, 256 images: {ms * 1e3:.0f} us per batch = {256 / ms * 1e3:.0f} images/s; {moved / 1e6:.1f} MB moved "
          f"({moved / nbytes.sum() * 3:.1f} B per pixel) = {moved / ms / 1e6:.1f} GB/s; H2D of the coefficients {coefs.numel() / 1e6:.1f} MB "
          f"against {nbytes.sum() / 1e6:.1f} MB of decoded RGB", flush=True)


def pipeline(paths, tmp, model, workers, gpu_jpeg, tag):
    """worker() over ALL shards as one partition -> (samples/s, output folder)."""
    from clip_retrieval_amd.worker import worker

    out = os.path.join(tmp, f"out-{model.replace('/', '_')}-{int(gpu_jpeg)}-{tag}")
    t0 = time.perf_counter()
    worker([0], input_dataset=paths, output_folder=out, output_partition_count=1, input_format="webdataset", batch_size=256,
           num_prepro_workers=workers, enable_text=False, enable_image=True, clip_model="random:" + model, gpu_resize=True, gpu_jpeg=gpu_jpeg)
    dt = time.perf_counter() - t0
    rows = sum(np.load(f, mmap_mode="r").shape[0] for f in glob.glob(out + "/img_emb/*.npy"))
    return rows / dt, out


SPLITS = (128, 256, 512)  # split_bytes of the split decode inside an interval
MODES = {"off": {}, "host entropy": {"gpu_jpeg": True}, "device entropy": {"gpu_huffman": True},
         **{f"device split {n}": {"gpu_huffman": True, "huffman_split": n} for n in SPLITS}}


def split_stage(files, dev, descs, offs, coefs, status, want):
    """The device stage on the batch without restart markers: serial (one wave per image) and every split size alternating in ONE
    run, each launch between its own events, medians; then the distribution of `rounds` over the distinct files."""
    import torch

    from clip_retrieval_amd import jpeg

    settings = (0,) + SPLITS
    rounds = torch.zeros(256, dtype=torch.int32, device="cuda")
    ms = {n: [] for n in settings}
    for rep in range(13):  # (the first pass of each setting is the warm-up)
        for n in settings:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            jpeg.entropy_device(0, dev, descs, offs, coefs, status, split_bytes=n)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms[n].append(e0.elapsed_time(e1))
            assert int(status.abs().sum()) == 0
            got = coefs.cpu().numpy()[int(descs["coef_off"][0]):int(descs["coef_off"][0]) + want.size] if rep == 0 else want
            assert np.array_equal(got, want)
    base = np.median(ms[0])
    for n in settings:
        v = ms[n]
        print(f"Huffman stage alone, 256 images without restart markers, {'serial (one wave per image)' if n == 0 else f'split {n}'}: median "
              f"{np.median(v):.2f} ms per batch of 12 alternating launches (min {min(v):.2f}, max {max(v):.2f}) = {base / np.median(v):.2f} x serial",
              flush=True)
    for n in SPLITS:
        jpeg.entropy_device(0, dev, descs, offs, coefs, status, split_bytes=n, max_rounds=4096, rounds_dev=rounds)
        r = rounds.cpu().numpy()[:64]  # (the batch repeats 64 distinct files)
        hist = ", ".join(f"{k}: {c}" for k, c in sorted(zip(*np.unique(r, return_counts=True))))
        over = int((r > jpeg.SPLIT_DEFAULT_ROUNDS).sum())
        print(f"rounds to the fixed point at split {n}, 64 files, max_rounds 4096: min {r.min()}, median {int(np.median(r))}, p99 "
              f"{int(np.percentile(r, 99))}, max {r.max()}; above the default cap of {jpeg.SPLIT_DEFAULT_ROUNDS}: {over} of 64 "
              f"({100 * over / 64:.1f} % would fall back); histogram {{{hist}}}", flush=True)


def huffman_stage(restart):
    """clipx_jpeg_entropy_device alone: 256 images, `restart` MCUs per interval (0: none, one wave per image)."""
    import torch
    from PIL import Image

    from clip_retrieval_amd import jpeg
    from clip_retrieval_amd.synth import synth_pixels_u8

    files = []
    for im in synth_pixels_u8(64, 256):
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="JPEG", quality=95, subsampling=2, restart_marker_blocks=restart)
        files.append(buf.getvalue())
    files = [files[i % 64] for i in range(256)]
    t0 = time.perf_counter()
    host = [jpeg.entropy_packed(f) for f in files]
    t1 = time.perf_counter()
    packed = [jpeg.scan_packed(f) for f in files]
    t2 = time.perf_counter()
    scans, descs, offs, coef_bytes = jpeg.pack_scans(packed, True)
    dev = scans.cuda()
    coefs = torch.empty(coef_bytes, dtype=torch.uint8, device="cuda")
    status = torch.empty(256, dtype=torch.int32, device="cuda")
    for _ in range(3):
        jpeg.entropy_device(0, dev, descs, offs, coefs, status)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        jpeg.entropy_device(0, dev, descs, offs, coefs, status)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    assert int(status.abs().sum()) == 0
    got, want = coefs.cpu().numpy(), jpeg.unpack(host[0])[1]
    assert np.array_equal(got[int(descs["coef_off"][0]):int(descs["coef_off"][0]) + want.size], want)
    intervals = int(packed[0][64:128].view(jpeg.SCAN_HEADER)[0]["nintervals"])
    print(f"Huffman stage alone, 256 images, {intervals} interval(s) per image: {ms:.2f} ms per batch = {256 / ms * 1e3:.0f} images/s "
          f"(events around the launch, mean of {reps}); one host core: entropy stage {256 / (t1 - t0):.0f} images/s, scan preparation "
          f"{256 / (t2 - t1):.0f} images/s; per image {np.mean([len(f) for f in files]) / 1024:.1f} KiB of file, {scans.numel() / 256 / 1024:.1f} KiB "
          f"of scan record, {np.mean([h.size for h in host]) / 1024:.1f} KiB of coefficient record", flush=True)
    if intervals == 1:
        split_stage(files, dev, descs, offs, coefs, status, want)


def reader_rate3(paths, workers, mode):
    """reader_rate in one of MODES."""
    import torch

    from clip_retrieval_amd import load_library
    from clip_retrieval_amd.encoder import resize_crop_device
    from clip_retrieval_amd.reader import DecodeRgbU8, WebdatasetReader
    from clip_retrieval_amd.runner import Sampler

    lib = load_library()
    r = WebdatasetReader(Sampler(0, 1), DecodeRgbU8(224, **MODES[mode]), None, paths, 256, workers, enable_text=False)
    t0 = time.perf_counter()
    n = taken = 0
    for b in r:
        jp = b.get("image_jpeg_scan") or b.get("image_jpeg")
        out = resize_crop_device(lib, 0, 224, b["image_raw"], None, jp)
        assert out.shape[0] == b["image_raw"]["hw"].shape[0]
        n += out.shape[0]
        taken += 0 if jp is None else len(jp["slots"])
    torch.cuda.synchronize()
    assert taken == (0 if mode == "off" else n)
    return n / (time.perf_counter() - t0)


def pipeline3(paths, tmp, model, workers, mode, tag):
    from clip_retrieval_amd.worker import worker

    out = os.path.join(tmp, f"out3-{model.replace('/', '_')}-{mode.replace(' ', '_')}-{tag}")
    t0 = time.perf_counter()
    switches = {("gpu_huffman_split" if k == "huffman_split" else k): v for k, v in MODES[mode].items()}
    worker([0], input_dataset=paths, output_folder=out, output_partition_count=1, input_format="webdataset", batch_size=256,
           num_prepro_workers=workers, enable_text=False, enable_image=True, clip_model="random:" + model, gpu_resize=True, **switches)
    dt = time.perf_counter() - t0
    rows = sum(np.load(f, mmap_mode="r").shape[0] for f in glob.glob(out + "/img_emb/*.npy"))
    return rows / dt, out


def alternate3(name, run, rounds):
    """The MODES alternating, `rounds` times after one untimed pass of each."""
    for mode in MODES:
        run(mode, "warm")
    rates = {mode: [] for mode in MODES}
    for i in range(rounds):
        for mode in MODES:
            rates[mode].append(run(mode, str(i)))
    for mode, v in rates.items():
        print(f"{name}, {mode}: median {np.median(v):.0f} samples/s of {rounds} alternating passes ({', '.join(f'{x:.0f}' for x in v)})", flush=True)
    off = np.median(rates["off"])
    print(f"{name}: " + ", ".join(f"{mode} / off = {np.median(v) / off:.3f}" for mode, v in rates.items() if mode != "off"), flush=True)


def huffman_legs(a, paths, tmp):
    for restart in (0, 16):  # 256 x 256 at 4:2:0 is 16 x 16 MCUs: 16 per interval is one interval per MCU row
        huffman_stage(restart)
    for w in sorted({a.few_workers, a.workers}):
        alternate3(f"reader + upload + GPU resize, {w} decode processes", lambda mode, tag, w=w: reader_rate3(paths, w, mode), a.rounds)
    for model in [m for m in a.models.split(",") if m]:
        outs = {}

        def run(mode, tag, model=model, outs=outs):
            rate, outs[mode] = pipeline3(paths, tmp, model, a.workers, mode, tag)
            return rate

        alternate3(f"pipeline worker() {model} images, {a.workers} decode processes, gpu_resize", run, a.rounds)
        embs = {mode: [np.load(f) for f in sorted(glob.glob(outs[mode] + "/img_emb/*.npy"))] for mode in MODES}
        same = all(len(embs[m]) == len(embs["off"]) and all(np.array_equal(x, y) for x, y in zip(embs[m], embs["off"])) for m in MODES)
        print(f"    {model}: embeddings of the {len(MODES)} settings {'equal' if same else 'DIFFER'}", flush=True)


def alternate(name, run, rounds):
    """off / on alternating, `rounds` times after one untimed pass of each (start-up of the decode processes, warm-up)."""
    run(False, "warm"), run(True, "warm")
    rates = {False: [], True: []}
    for i in range(rounds):
        for on in (False, True):
            rates[on].append(run(on, str(i)))
    for on in (False, True):
        v = rates[on]
        print(f"{name}, gpu_jpeg {'on ' if on else 'off'}: median {np.median(v):.0f} samples/s of {rounds} alternating passes ({', '.join(f'{x:.0f}' for x in v)})", flush=True)
    print(f"{name}: on / off = {np.median(rates[True]) / np.median(rates[False]):.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--samples", type=int, default=32768, help="JPEG members in all (8 shards); every timed pass reads all of them")
    ap.add_argument("--few-workers", type=int, default=4, help="a second reader leg with this many decode processes")
    ap.add_argument("--rounds", type=int, default=3, help="alternating off / on passes per leg")
    ap.add_argument("--models", default="ViT-B/32,ViT-L/14")
    ap.add_argument("--legs", default="jpeg", choices=("jpeg", "huffman", "all"), help="jpeg: legs 1 - 3; huffman: legs 4 - 6")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    paths, jpegs = make_shards(tmp, 8, a.samples // 8)
    if not os.environ.get("CLIP_BPE_PATH"):  # load_clip builds a tokenizer even for an image-only run: a stand-in merges file
        import gzip

        os.environ["CLIP_BPE_PATH"] = os.path.join(tmp, "bpe_simple_vocab_16e6.txt.gz")
        with gzip.open(os.environ["CLIP_BPE_PATH"], "wt", encoding="utf-8") as f:
            f.write("#version: 0.2\nt h\nth e</w>\no f</w>\np h\n")
    print(f"host cores visible: {os.cpu_count()}; decode processes: {a.workers}", flush=True)
    if a.legs in ("huffman", "all"):
        huffman_legs(a, paths, tmp)
    if a.legs == "huffman":
        shutil.rmtree(tmp, ignore_errors=True)
        return
    entropy_rate(jpegs)
    pixel_stage(jpegs)
    for w in sorted({a.few_workers, a.workers}):  # few processes: the decode is the bound; many: the parent process is
        alternate(f"reader + upload + GPU resize, {w} decode processes", lambda on, tag, w=w: reader_rate(paths, w, on), a.rounds)
    for model in [m for m in a.models.split(",") if m]:
        outs = {}

        def run(on, tag, model=model, outs=outs):
            rate, outs[on] = pipeline(paths, tmp, model, a.workers, on, tag)
            return rate

        alternate(f"pipeline worker() {model} images, {a.workers} decode processes, gpu_resize", run, a.rounds)
        same = all(np.array_equal(np.load(x), np.load(y)) for x, y in zip(*(sorted(glob.glob(outs[o] + "/img_emb/*.npy")) for o in (False, True))))
        print(f"    {model}: embeddings with the switch on {'equal' if same else 'DIFFER FROM'} those with it off", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
