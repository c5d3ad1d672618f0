"""The Huffman stage of the GPU JPEG decoder without a GPU (`gpu_huffman`): the host preparation of csrc/jpegx_scan.h and
the interval decoder the kernel instantiates, run on the CPU under the sanitizers against the host entropy stage
(csrc/jpegx_entropy.h, itself pinned to Pillow by test_jpeg_cpu.py); the C ABI of the preparation; and the reader carrying scans
without changing a byte when the switch is off."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_inputs as J
from test_jpeg_cpu import deferred_inputs

ROOT = J.ROOT
CSRC = os.path.join(ROOT, "clip-retrieval_amd", "csrc")


def mutants(n=2000):
    """The single-byte mutants of test_jpeg_cpu.py::test_entropy_stage_under_sanitizers (seed 7, three small files), the first n."""
    rng = np.random.default_rng(7)
    small = [J.encode(J.content("noise", 16, 16, 3), 2, 75, False, 1), J.encode(J.content("checker", 17, 9, 4), 0, 30, True, 0),
             J.encode(J.content("gradient", 9, 16, 5), "L", 95, False, 3)]
    out = []
    for i in range(n):
        b = bytearray(small[i % 3])
        b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    return out


def test_scan_stage_under_sanitizers(tmp_path):
    """tools/jpeg_scan_check.cpp (its own main, only the two headers) built with -fsanitize=address,undefined and run as a child over
    the 146 accepted files, the deferred set with its prefixes and the 2 000 seeded mutants.  Per file: the record is prepared into a
    buffer of exactly the queried size (guards behind a second one), every interval is decoded on its own in reverse order, the host
    stage takes the file exactly when the preparation does and every interval is clean, and then the records are byte-equal."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    files = tmp_path / "files"
    files.mkdir()
    n_taken = len(J.cases())
    for i, (_, data) in enumerate(J.cases()):
        (files / f"a{i:04d}.bin").write_bytes(data)
    n_deferred = len(deferred_inputs())
    for i, (_, data) in enumerate(deferred_inputs()):
        (files / f"d{i:04d}.bin").write_bytes(data)
    for i, data in enumerate(mutants()):
        (files / f"m{i:04d}.bin").write_bytes(data)
    exe = str(tmp_path / "jpeg_scan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(ROOT, "tools", "jpeg_scan_check.cpp"), "-o", exe]
    build = subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe, str(files)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("jpeg scan ok") and "FAILED" not in run.stdout
    counts = {ln.split()[1]: ln.split()[2:] for ln in run.stdout.splitlines() if ln.startswith("prefix ")}
    print(counts)
    assert n_taken == 146 and counts["a"] == [f"{n_taken}/{n_taken}", str(n_taken), "0"], counts  # all taken, all clean
    assert counts["d"][0] == f"0/{n_deferred}", counts  # none taken
    assert counts["m"][0].endswith("/2000"), counts
    reached, unclean = int(counts["m"][1]), int(counts["m"][2])
    assert reached >= 1400 and unclean >= 300, counts  # the mutants do reach the interval decoder, and it does refuse some


def test_header_has_no_hip_and_is_in_the_makefile():
    text = open(os.path.join(CSRC, "jpegx_scan.h"), encoding="utf-8").read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ['"jpegx_entropy.h"'], includes  # system headers come through it
    for word in ("__global__", "hipStream", "hipError", "hipMalloc", "hipMemcpy", "hipLaunch", "<<<", "hip_runtime"):
        assert word not in text, word
    # __host__ __device__ appears once: in the macro that is empty without hipcc
    assert text.count("__device__") == 1 and "#define JPEGX_HD __host__ __device__" in text and "#define JPEGX_HD\n" in text
    mk = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "jpeg_huff_kernels.hip" in mk and "jpegx_scan.h" in mk
    kernel = open(os.path.join(CSRC, "jpeg_huff_kernels.hip"), encoding="utf-8").read()
    assert '#include "jpegx_scan.h"' in kernel and "asm" not in kernel and "__shared__" not in kernel


def _scan_stages(lib, data, fill=0xA5):
    from clip_retrieval_amd import jpeg

    desc = np.zeros(1, dtype=jpeg.JPEG_DESC)
    desc.view(np.uint8)[:] = fill
    need = C.c_size_t(12345)
    p = lib.clipx_jpeg_scan_probe_host(data, len(data), 8192, desc.ctypes.data, C.byref(need))
    probed = desc.copy()
    size = need.value if p == jpeg.TAKEN else 4096
    desc.view(np.uint8)[:] = fill
    rec = np.full(size + 64, fill, dtype=np.uint8)
    e = lib.clipx_jpeg_scan_host(data, len(data), 8192, desc.ctypes.data, rec.ctypes.data, size)
    untouched = bool((rec == fill).all() and (desc.view(np.uint8) == fill).all())
    if p != jpeg.TAKEN:
        untouched = untouched and need.value == 12345 and bool((probed.view(np.uint8) == fill).all())
    return p, e, untouched, rec, size, desc


def test_scan_abi_takes_the_class_and_writes_nothing_on_a_deferral(lib):
    from clip_retrieval_amd import jpeg

    for name, data in deferred_inputs():
        p, e, untouched, _, _, _ = _scan_stages(lib, data)
        assert p in (jpeg.TAKEN, jpeg.DEFERRED) and e == jpeg.DEFERRED, (name, p, e)
        assert untouched, f"{name}: a deferral wrote to the descriptor or the record"
        assert jpeg.scan_packed(data, lib=lib) is None
    for name, data in J.cases():
        p, e, untouched, rec, size, desc = _scan_stages(lib, data)
        assert (p, e) == (jpeg.TAKEN, jpeg.TAKEN) and not untouched and (rec[size:] == 0xA5).all(), name
        packed = jpeg.scan_packed(data, lib=lib)
        want = jpeg.entropy(data, lib=lib)[0]
        want["coef_off"] = 0
        assert packed.size == 64 + size and np.array_equal(packed[64:], rec[:size]) and packed[:64].tobytes() == want.tobytes(), name
        head = packed[64:128].view(jpeg.SCAN_HEADER)[0]
        assert head["total_bytes"] == size and size % 16 == 0 and head["file_bytes"] == len(data) and 1 <= head["ntables"] <= 6
        mcus = (int(want[0]["bw"][0]) // int(want[0]["hs"])) * (int(want[0]["bh"][0]) // int(want[0]["vs"]))
        rst = int(want[0]["restart"])
        assert head["nintervals"] == (-(-mcus // rst) if rst else 1), name
        assert jpeg.scan_file(packed[64:]) == data, name  # the file as it is: what a late Pillow decode reads
    # max_side is part of the class
    big = J.encode(J.content("gradient", 33, 15, 0), 2, 90, False, 0)
    assert jpeg.scan_packed(big, max_side=33, lib=lib) is not None and jpeg.scan_packed(big, max_side=32, lib=lib) is None


def test_pack_scans_layout(lib):
    from clip_retrieval_amd import jpeg

    items = [jpeg.scan_packed(d, lib=lib) for _, d in J.cases()[5::29]]
    buf, descs, offs, coef_bytes = jpeg.pack_scans(items)
    assert offs.shape == (len(items) + 1,) and offs[0] == 0 and offs[-1] == buf.numel() and (offs % 16 == 0).all()
    end = 0
    for k, it in enumerate(items):
        assert np.array_equal(buf.numpy()[offs[k]:offs[k] + it.size - 64], it[64:])
        assert descs["coef_off"][k] == end and end % 16 == 0  # records of the coefficient buffer: one behind the other
        end += (jpeg.record_bytes(descs[k]) + 15) & ~15
    assert coef_bytes == end


# ---- the reader ----------------------------------------------------------------------------------------------------------------
def _raw(key, data):
    return {"key": key, "image": data, "text": None, "metadata": None}


def _golden(name):
    with open(os.path.join(J.GOLDEN, "test_images", name), "rb") as f:
        return f.read()


def test_decode_sample_and_collate_carry_scans(lib):
    from PIL import Image

    from clip_retrieval_amd import jpeg, reader as R

    huff, off = R.DecodeRgbU8(224, gpu_huffman=True), R.DecodeRgbU8(224)
    assert huff.gpu_huffman and huff.gpu_jpeg and not off.gpu_huffman and R.decode_rgb_u8.gpu_huffman is False
    assert R.DecodeRgbU8(224, gpu_jpeg=True).gpu_huffman is False
    base, prog = _golden("123_456.jpg"), _golden("208_495.jpg")
    s_base = R._decode_sample(_raw("b", base), huff, None, True, False, False)
    s_prog = R._decode_sample(_raw("p", prog), huff, None, True, False, False)
    o_base = R._decode_sample(_raw("b", base), off, None, True, False, False)
    o_prog = R._decode_sample(_raw("p", prog), off, None, True, False, False)
    # a deferred file: the old result; a baseline member: its scan, never coefficients
    assert sorted(s_prog) == ["image_filename", "image_raw"] and np.array_equal(s_prog["image_raw"], o_prog["image_raw"])
    assert sorted(s_base) == ["image_filename", "image_jpeg_scan"] and s_base["image_filename"] == "b"
    packed = s_base["image_jpeg_scan"]
    assert packed.dtype == np.uint8 and np.array_equal(packed, jpeg.scan_packed(base, lib=lib)) and jpeg.scan_file(packed[64:]) == base
    desc = packed[:64].view(jpeg.JPEG_DESC)[0]
    assert (int(desc["height"]), int(desc["width"])) == o_base["image_raw"].shape[:2]
    assert R._decode_sample(_raw("x", b"nonsense"), huff, None, True, False, False) is None
    assert "image_raw" in R._decode_sample(_raw("b", base), R.DecodeRgbU8(224, max_side=200, gpu_huffman=True), None, True, False, False)

    # a mixed batch: the image_raw layout with the taken images' bytes reserved, exactly as image_raw would have sized them
    second = R._decode_sample(_raw("b2", _golden("456_123.jpg")), huff, None, True, False, False)
    o_second = R._decode_sample(_raw("b2", _golden("456_123.jpg")), off, None, True, False, False)
    batch = R._collate([s_prog, s_base, second, dict(s_prog, image_filename="p2")], True, False, False, False)
    plain = R._collate([o_prog, o_base, o_second, dict(o_prog, image_filename="p2")], True, False, False, False)
    assert sorted(batch) == ["image_filename", "image_jpeg_scan", "image_raw"]
    raw, sc = batch["image_raw"], batch["image_jpeg_scan"]
    assert np.array_equal(raw["hw"], plain["image_raw"]["hw"]) and raw["hw"].dtype == np.int32
    assert np.array_equal(raw["offsets"], plain["image_raw"]["offsets"]) and raw["pixels"].numel() == plain["image_raw"]["pixels"].numel()
    flat, want = raw["pixels"].numpy(), plain["image_raw"]["pixels"].numpy()
    for i in (0, 3):
        o, n = int(raw["offsets"][i]), int(raw["hw"][i, 0]) * int(raw["hw"][i, 1]) * 3
        assert np.array_equal(flat[o:o + n], want[o:o + n])
    assert sorted(sc) == ["coef_bytes", "descs", "names", "offs", "scans", "slots"]
    assert sc["slots"].tolist() == [1, 2] and sc["names"] == ["b", "b2"] and sc["descs"].dtype == jpeg.JPEG_DESC and sc["descs"].shape == (2,)
    assert batch["image_filename"] == ["p", "b", "b2", "p2"]
    for k, s in enumerate((s_base, second)):
        rec = s["image_jpeg_scan"][64:]
        assert np.array_equal(sc["scans"].numpy()[sc["offs"][k]:sc["offs"][k] + rec.size], rec)
    assert sc["coef_bytes"] == sum((jpeg.record_bytes(d) + 15) & ~15 for d in sc["descs"])
    # coefficients and scans never share a batch
    coef = R._decode_sample(_raw("b", base), R.DecodeRgbU8(224, gpu_jpeg=True), None, True, False, False)
    with pytest.raises(ValueError):
        R._collate([s_base, coef], True, False, False, False)


def test_switch_off_leaves_samples_and_batches_as_they_are(lib):
    """gpu_huffman off (the default): `_decode_sample` and `_collate` give today's keys and bytes, with gpu_jpeg on and off --
    compared with what the entry points of the coefficient path (jpeg.entropy_packed / jpeg.pack_records) and Pillow give."""
    from PIL import Image

    from clip_retrieval_amd import jpeg, reader as R

    files = [("b", _golden("123_456.jpg")), ("p", _golden("208_495.jpg")), ("c", _golden("456_123.jpg"))]
    for pre in (R.DecodeRgbU8(224), R.DecodeRgbU8(224, gpu_jpeg=True), R.DecodeRgbU8(224, gpu_jpeg=True, gpu_huffman=False)):
        samples = [R._decode_sample(_raw(k, d), pre, None, True, False, False) for k, d in files]
        for (k, d), s in zip(files, samples):
            taken = jpeg.entropy_packed(d, lib=lib) if pre.gpu_jpeg else None
            if taken is not None:
                assert sorted(s) == ["image_filename", "image_jpeg"] and np.array_equal(s["image_jpeg"], taken)
            else:
                assert sorted(s) == ["image_filename", "image_raw"]
                assert np.array_equal(s["image_raw"], np.asarray(Image.open(io.BytesIO(d)).convert("RGB")))
        batch = R._collate(samples, True, False, False, False)
        assert sorted(batch) == (["image_filename", "image_jpeg", "image_raw"] if pre.gpu_jpeg else ["image_filename", "image_raw"])
        assert sorted(batch["image_raw"]) == ["hw", "offsets", "pixels"]
        if pre.gpu_jpeg:
            assert sorted(batch["image_jpeg"]) == ["coefs", "descs", "slots"] and batch["image_jpeg"]["slots"].tolist() == [0, 2]
            coefs, descs = jpeg.pack_records([samples[0]["image_jpeg"], samples[2]["image_jpeg"]])
            assert np.array_equal(batch["image_jpeg"]["coefs"].numpy(), coefs.numpy()) and batch["image_jpeg"]["descs"].tobytes() == descs.tobytes()


def test_decode_pool_carries_scans(tmp_path):
    """Through the decode processes (no GPU in them): the scan records come back through the arena byte for byte."""
    import tarfile

    from clip_retrieval_amd import jpeg, reader as R
    from clip_retrieval_amd.runner import Sampler

    shard = str(tmp_path / "s.tar")
    names = ["123_456.jpg", "208_495.jpg", "456_123.jpg", "321_421.jpg", "123_456.jpg"]
    with tarfile.open(shard, "w") as tf:
        for i, n in enumerate(names):
            data = _golden(n)
            info = tarfile.TarInfo(f"{i:03d}.jpg")
            info.size = len(data)
            tf.addfile(info, io.BytesIO(data))
    huff = R.DecodeRgbU8(224, gpu_huffman=True)
    try:
        r = R.WebdatasetReader(Sampler(0, 1), huff, None, [shard], 5, 2, enable_text=False)
        r.reference_batch_order = False
        batches = list(r)
    finally:
        R._DecodePool.shutdown()
    assert len(batches) == 1
    b = batches[0]
    assert "image_jpeg" not in b and b["image_jpeg_scan"]["slots"].tolist() == [0, 2, 4] and b["image_filename"] == [f"{i:03d}" for i in range(5)]
    assert b["image_jpeg_scan"]["names"] == ["000", "002", "004"]
    sc = b["image_jpeg_scan"]
    for k, n in enumerate(("123_456.jpg", "456_123.jpg", "123_456.jpg")):
        rec = jpeg.scan_packed(_golden(n))[64:]
        assert np.array_equal(sc["scans"].numpy()[sc["offs"][k]:sc["offs"][k] + rec.size], rec)
        assert jpeg.scan_file(sc["scans"].numpy()[sc["offs"][k]:sc["offs"][k + 1]]) == _golden(n)


def test_late_decode_is_the_deferred_branch(capsys):
    """reader.late_decode -- what encoder.resize_crop_device calls for a file the device refused -- gives the pixels of the deferred
    branch of `_decode_sample`, and None with that branch's skip line where Pillow raises or the size is not the reserved one."""
    from clip_retrieval_amd import reader as R

    pre = R.DecodeRgbU8(224)
    base = _golden("123_456.jpg")
    want = R._decode_sample(_raw("k", base), pre, None, True, False, False)["image_raw"]
    h, w = want.shape[:2]
    assert np.array_equal(R.late_decode("k", base, pre, h, w), want)
    assert R.late_decode("k", base, pre, h + 1, w) is None
    assert R.late_decode("t", base[:len(base) // 2], pre, h, w) is None and R._decode_sample(_raw("t", base[:len(base) // 2]), pre, None, True, False, False) is None
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln]
    assert len(lines) == 3 and all(ln.startswith("Failed to load image ") and ln.endswith(" Skipping.") for ln in lines)
    assert lines[1] == lines[2]  # the truncated file: the same line from both branches
