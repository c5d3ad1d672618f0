"""Baseline JPEG decode in two stages: the host half of the binding.

`entropy()` runs the entropy stage of lib/libclipx.so (csrc/jpegx_entropy.h: markers + Huffman -> int16 DCT coefficients) on one
file's bytes.  It makes no HIP call, so the readers' decode processes use it without a GPU.  A file outside the accepted class --
or one that does not parse cleanly -- is DEFERRED (`None`): the caller decodes it with Pillow as before.  `pixels_device()` is the
device half: records -> packed RGB, bit-identical to Pillow (csrc/jpeg_kernels.hip).

With the Huffman stage on the device (`gpu_huffman`): `scan_packed()` only parses markers (csrc/jpegx_scan.h, no HIP call either) and
`entropy_device()` turns the scan records of a batch into the same records on the GPU (csrc/jpeg_huff_kernels.hip), with a status
per image that is non-zero exactly where `entropy()` would have deferred the file.
"""

import ctypes as C

import numpy as np

from ._lib import check, load_library

# clipx_jpeg_desc of include/clipx.h, 64 bytes
JPEG_DESC = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("bw", "<i4", (3,)),
                      ("bh", "<i4", (3,)), ("blocks", "<i4"), ("restart", "<i4"), ("pad", "<i4"), ("coef_off", "<i8")])
assert JPEG_DESC.itemsize == 64
TABLE_BYTES = 3 * 64 * 2  # the three quantisation tables at the head of a record
DEFERRED, TAKEN = 0, 1


def record_bytes(desc):
    return TABLE_BYTES + int(desc["blocks"]) * 128


def probe(data, max_side=8192, lib=None):
    """(descriptor, record bytes) of a file of the accepted class, from its markers up to the SOF; None = deferred."""
    lib = lib or load_library()
    desc = np.zeros(1, dtype=JPEG_DESC)
    need = C.c_size_t(0)
    buf = bytes(data)
    rc = lib.clipx_jpeg_probe_host(buf, len(buf), int(max_side), desc.ctypes.data, C.byref(need))
    if rc < 0:
        check(lib, rc, "clipx")
    return (desc, need.value) if rc == TAKEN else None


def entropy_packed(data, max_side=8192, lib=None):
    """One uint8 array [64 bytes of descriptor | record] of a file of the accepted class -- the form in which a sample travels from
    a decode process to the batch (`image_jpeg` of reader._decode_sample) -- or None = deferred."""
    lib = lib or load_library()
    buf = bytes(data)
    got = probe(buf, max_side, lib)
    if got is None:
        return None
    need = got[1]
    packed = np.empty(JPEG_DESC.itemsize + need, dtype=np.uint8)
    rc = lib.clipx_jpeg_entropy_host(buf, len(buf), int(max_side), packed.ctypes.data, packed.ctypes.data + JPEG_DESC.itemsize, need)
    if rc < 0:
        check(lib, rc, "clipx")
    return packed if rc == TAKEN else None


def unpack(packed):
    """(descriptor [1] of JPEG_DESC, record) views of an entropy_packed() array."""
    return packed[:JPEG_DESC.itemsize].view(JPEG_DESC), packed[JPEG_DESC.itemsize:]


def entropy(data, max_side=8192, lib=None):
    """(descriptor [1] of JPEG_DESC, record uint8 [record_bytes]) of a file of the accepted class; None = deferred."""
    packed = entropy_packed(data, max_side, lib)
    return None if packed is None else unpack(packed)


def pack_records(packed, pin=False):
    """The entropy_packed() arrays of a batch in ONE (page-locked) byte buffer, each on a 16-byte boundary -> (torch uint8 buffer,
    descriptors [n] with coef_off pointing at each record)."""
    import torch  # pylint: disable=import-outside-toplevel

    sizes = np.asarray([(r.size + 15) & ~15 for r in packed], dtype=np.int64)
    starts = np.zeros(len(packed), dtype=np.int64)
    np.cumsum(sizes[:-1], out=starts[1:])
    buf = torch.empty(int(sizes.sum()), dtype=torch.uint8, pin_memory=bool(pin))
    flat = buf.numpy()
    for r, o in zip(packed, starts):
        flat[o:o + r.size] = r
    descs = np.stack([r[:JPEG_DESC.itemsize] for r in packed]).view(JPEG_DESC).reshape(-1)
    descs["coef_off"] = starts + JPEG_DESC.itemsize
    return buf, descs


def scan_packed(data, max_side=8192, lib=None):
    """One uint8 array [64 bytes of descriptor | scan record] of a file of the accepted class whose entropy-coded bytes end in the
    markers they should -- the form in which a sample travels when the Huffman stage runs on the device (`image_jpeg_scan` of
    reader._decode_sample; csrc/jpegx_scan.h) -- or None = deferred.  No Huffman decoding happens here."""
    lib = lib or load_library()
    buf = bytes(data)
    desc = np.zeros(1, dtype=JPEG_DESC)
    need = C.c_size_t(0)
    rc = lib.clipx_jpeg_scan_probe_host(buf, len(buf), int(max_side), desc.ctypes.data, C.byref(need))
    if rc < 0:
        check(lib, rc, "clipx")
    if rc != TAKEN:
        return None
    packed = np.empty(JPEG_DESC.itemsize + need.value, dtype=np.uint8)
    rc = lib.clipx_jpeg_scan_host(buf, len(buf), int(max_side), packed.ctypes.data, packed.ctypes.data + JPEG_DESC.itemsize, need.value)
    if rc < 0:
        check(lib, rc, "clipx")
    return packed if rc == TAKEN else None


SCAN_HEADER = np.dtype([("magic", "<u4"), ("total_bytes", "<u4"), ("file_bytes", "<u4"), ("nintervals", "<i4"), ("ntables", "<i4"),
                        ("dc_tab", "<i4", (3,)), ("ac_tab", "<i4", (3,)), ("pad", "<i4", (5,))])  # ScanHeader of csrc/jpegx_scan.h
assert SCAN_HEADER.itemsize == 64
HUFF_BYTES, INTERVAL_BYTES = 2448, 16


def scan_file(record):
    """The file's own bytes out of a scan record (a scan_packed() array behind its descriptor, or a record of pack_scans()'s
    buffer): what a late Pillow decode reads."""
    record = np.asarray(record, dtype=np.uint8)
    h = record[:SCAN_HEADER.itemsize].view(SCAN_HEADER)[0]
    at = SCAN_HEADER.itemsize + TABLE_BYTES + int(h["ntables"]) * HUFF_BYTES + int(h["nintervals"]) * INTERVAL_BYTES
    return record[at:at + int(h["file_bytes"])].tobytes()


def pack_scans(packed, pin=False):
    """The scan_packed() arrays of a batch in ONE (page-locked) byte buffer -> (torch uint8 buffer of the scan records, descriptors
    [n] with coef_off laid out for the records the device stage will WRITE, scan offsets int64 [n + 1], bytes of that coefficient
    buffer).  Record i of the scans lies in [offs[i], offs[i + 1]), each on a 16-byte boundary."""
    import torch  # pylint: disable=import-outside-toplevel

    sizes = np.asarray([(r.size - JPEG_DESC.itemsize + 15) & ~15 for r in packed], dtype=np.int64)
    offs = np.zeros(len(packed) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offs[1:])
    buf = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=bool(pin))
    flat = buf.numpy()
    for r, o in zip(packed, offs):
        flat[o:o + r.size - JPEG_DESC.itemsize] = r[JPEG_DESC.itemsize:]
    descs = np.stack([r[:JPEG_DESC.itemsize] for r in packed]).view(JPEG_DESC).reshape(-1) if len(packed) else np.zeros(0, JPEG_DESC)
    rec = (TABLE_BYTES + descs["blocks"].astype(np.int64) * 128 + 15) & ~15
    descs["coef_off"] = np.cumsum(rec) - rec
    return buf, descs, offs, int(rec.sum())


JPEG_SPLIT = np.dtype([("split_bytes", "<i4"), ("max_rounds", "<i4"), ("reserved", "<i4", (2,))])  # clipx_jpeg_split of include/clipx.h
SPLIT_SIZES = (0, 32, 64, 128, 256, 512, 1024)
SPLIT_DEFAULT_ROUNDS = 16  # DEFAULT_MAX_ROUNDS of csrc/jpegx_split.h: what max_rounds=0 stands for


def _split_arg(split_bytes, max_rounds):
    if int(split_bytes) not in SPLIT_SIZES or int(max_rounds) < 0:
        raise ValueError("split_bytes is 0 or a power of two 32 .. 1024, max_rounds is 0 (the default) or >= 1")
    arg = np.zeros(1, dtype=JPEG_SPLIT)
    arg["split_bytes"], arg["max_rounds"] = int(split_bytes), int(max_rounds)
    return arg


def entropy_split_host(scan, desc, split_bytes, max_rounds=0, lib=None):
    """The split Huffman decode of csrc/jpegx_split.h on the host, lanes as a loop (no GPU): `scan` is ONE scan record (a
    scan_packed() array behind its 64-byte descriptor), `desc` its descriptor -> (status, record uint8 [record_bytes], rounds), what
    the device entry writes for that image (rounds: 0 not split, r >= 2 rounds taken, -r gave up after r rounds and decoded serially)."""
    lib = lib or load_library()
    desc = np.ascontiguousarray(desc, dtype=JPEG_DESC).reshape(-1)[:1].copy()
    aligned = np.empty(np.asarray(scan).size + 16, dtype=np.uint8)
    at = (-aligned.ctypes.data) & 15
    rec = aligned[at:at + np.asarray(scan).size]
    rec[:] = np.asarray(scan, dtype=np.uint8)
    out = np.empty(record_bytes(desc[0]), dtype=np.uint8)
    arg = _split_arg(split_bytes, max_rounds)
    status, rounds = C.c_int32(-1), C.c_int32(0)
    check(lib, lib.clipx_jpeg_entropy_split_host(rec.ctypes.data, rec.size, desc.ctypes.data, arg.ctypes.data, out.ctypes.data, out.size,
                                                 C.byref(status), C.byref(rounds)), "clipx")
    return status.value, out, rounds.value


def entropy_device(device, scans_dev, descs, scan_offs, coefs_dev, status_dev, stream=None, lib=None, split_bytes=0, max_rounds=0,
                   rounds_dev=None):
    """Run the Huffman stage on the device: scan record i (bytes [scan_offs[i], scan_offs[i + 1]) of the device tensor `scans_dev`)
    becomes the record pixels_device reads at descs[i].coef_off of `coefs_dev`; status_dev (device int32 [>= n]) gets 0 per clean
    image and a reason code per image the host stage would have deferred.  Asynchronous on `stream` (a hipStream_t value; None:
    torch's current).  The tensors' extents are checked here: the C entry point takes bare pointers."""
    import torch  # pylint: disable=import-outside-toplevel

    lib = lib or load_library()
    descs = np.ascontiguousarray(descs, dtype=JPEG_DESC)
    scan_offs = np.ascontiguousarray(scan_offs, dtype=np.int64)
    n = descs.shape[0]
    if scan_offs.shape != (n + 1,):
        raise ValueError("n + 1 scan offsets for n descriptors")
    if scans_dev.dtype != torch.uint8 or coefs_dev.dtype != torch.uint8 or status_dev.dtype != torch.int32:
        raise ValueError("scan and coefficient buffers are uint8 tensors, the status array is int32")
    if not (scans_dev.is_contiguous() and coefs_dev.is_contiguous() and status_dev.is_contiguous()):
        raise ValueError("contiguous tensors only")
    if n and (scan_offs[0] < 0 or (np.diff(scan_offs) < 0).any() or scan_offs[-1] > scans_dev.numel()):
        raise ValueError("a scan record lies outside the scan buffer")
    rec_end = descs["coef_off"] + TABLE_BYTES + descs["blocks"].astype(np.int64) * 128
    if n and (descs["coef_off"].min() < 0 or descs["blocks"].min() < 0 or rec_end.max() > coefs_dev.numel()):
        raise ValueError("a JPEG record lies outside the coefficient buffer")
    if status_dev.numel() < n:
        raise ValueError("one status word per image")
    st = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", device)).cuda_stream
    if split_bytes or max_rounds or rounds_dev is not None:  # the split decode inside an interval
        arg = _split_arg(split_bytes, max_rounds)
        if rounds_dev is not None and (rounds_dev.dtype != torch.int32 or not rounds_dev.is_contiguous() or rounds_dev.numel() < n):
            raise ValueError("rounds_dev is a contiguous int32 tensor with one word per image")
        check(lib, lib.clipx_jpeg_entropy_split_device(device, C.c_void_p(scans_dev.data_ptr()), descs.ctypes.data, scan_offs.ctypes.data, n,
                                                       C.c_void_p(coefs_dev.data_ptr()), C.c_void_p(status_dev.data_ptr()), arg.ctypes.data,
                                                       C.c_void_p(rounds_dev.data_ptr()) if rounds_dev is not None else None,
                                                       C.c_void_p(st) if st else None), "clipx")
        return
    check(lib, lib.clipx_jpeg_entropy_device(device, C.c_void_p(scans_dev.data_ptr()), descs.ctypes.data, scan_offs.ctypes.data, n,
                                             C.c_void_p(coefs_dev.data_ptr()), C.c_void_p(status_dev.data_ptr()),
                                             C.c_void_p(st) if st else None), "clipx")


def pixels_device(device, coefs_dev, descs, pixels_dev, offsets, stream=None, lib=None):
    """Run the pixel stage: image i of `descs` (its record at descs[i].coef_off of the device tensor `coefs_dev`) becomes packed RGB
    at byte offsets[i] of the device tensor `pixels_dev`.  Asynchronous on `stream` (a hipStream_t value; None: torch's current).
    Both tensors' extents are checked here: the C entry point takes bare pointers."""
    import torch  # pylint: disable=import-outside-toplevel

    lib = lib or load_library()
    descs = np.ascontiguousarray(descs, dtype=JPEG_DESC)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.shape != (descs.shape[0],):
        raise ValueError("one pixel offset per descriptor")
    if coefs_dev.dtype != torch.uint8 or pixels_dev.dtype != torch.uint8:
        raise ValueError("coefficient and pixel buffers are uint8 tensors")
    rec_end = descs["coef_off"] + TABLE_BYTES + descs["blocks"].astype(np.int64) * 128
    if descs.size and (descs["coef_off"].min() < 0 or descs["blocks"].min() < 0 or rec_end.max() > coefs_dev.numel()):
        raise ValueError("a JPEG record lies outside the coefficient buffer")
    pix_end = offsets + descs["height"].astype(np.int64) * descs["width"] * 3
    if descs.size and (offsets.min() < 0 or min(descs["height"].min(), descs["width"].min()) < 1 or pix_end.max() > pixels_dev.numel()):
        raise ValueError("a decoded image lies outside the pixel buffer")
    st = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", device)).cuda_stream
    check(lib, lib.clipx_jpeg_pixels_device(device, C.c_void_p(coefs_dev.data_ptr()), descs.ctypes.data, descs.shape[0],
                                            C.c_void_p(pixels_dev.data_ptr()), offsets.ctypes.data, C.c_void_p(st) if st else None), "clipx")
