"""Inputs of the JPEG decoder tests (test_jpeg_cpu.py, test_jpeg_gpu.py): the accepted class by construction, written with
Pillow in the test process, plus the two baseline goldens.  Not a test module."""
import functools
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_clip_inference")
BASELINE_GOLDENS = ("123_456.jpg", "456_123.jpg")
PROGRESSIVE_GOLDENS = ("208_495.jpg", "321_421.jpg", "389_535.jpg", "416_264.jpg", "524_316.jpg")

# (width, height): odd and even on both axes, below / at / above one block and one MCU, widths whose halved extent is <= 2
SIZES = ((1, 1), (3, 4), (4, 3), (5, 8), (8, 5), (9, 16), (15, 17), (16, 16), (17, 9), (33, 15), (16, 33), (131, 250))
SAMPLINGS = (0, 1, 2, "L")  # Pillow's `subsampling` (4:4:4, 4:2:2, 4:2:0) and mode L
QUALITIES = (5, 30, 95, 100)
RESTARTS = (0, 1, 3)
CONTENTS = ("noise", "gradient", "checker")


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    # black / white / saturated colours in cells of 1 .. 3 pixels: the inverse DCT overshoots, the range limit is hit
    colours = np.asarray([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255)], np.uint8)
    cell = 1 + seed % 3
    y, x = np.mgrid[0:h, 0:w]
    return colours[((x // cell) + 3 * (y // cell) + seed) % len(colours)]


def encode(arr, sampling, quality, optimize, restart):
    from PIL import Image, ImageFile

    buf = io.BytesIO()
    kw = {"quality": quality, "optimize": optimize, "progressive": False, "restart_marker_blocks": restart}
    # an optimised file must fit Pillow's encoder buffer in one piece ("Suspension not allowed here"): noise at quality 100 does not
    # fit the default, so the buffer is sized for the worst case while this file is written
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 8 * arr.shape[0] * arr.shape[1] + 4096)
    try:
        if sampling == "L":
            Image.fromarray(arr[..., 1]).save(buf, "JPEG", **kw)
        else:
            Image.fromarray(arr).save(buf, "JPEG", subsampling=sampling, **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, jpeg bytes)]: every size x sampling x content; quality, optimize and restart interval rotate so that every pair of
    values of two parameters occurs (checked by enumeration when the rotation was chosen)."""
    out, i = [], 0
    for w, h in SIZES:
        for s in SAMPLINGS:
            for kind in CONTENTS:
                q, opt, rst = QUALITIES[(i + i // 12) % 4], bool((i // 5) % 2), RESTARTS[(i // 4 + i // 12) % 3]
                out.append((f"{w}x{h}-s{s}-{kind}-q{q}-o{int(opt)}-r{rst}", encode(content(kind, w, h, i), s, q, opt, rst)))
                i += 1
    for name in BASELINE_GOLDENS:
        with open(os.path.join(GOLDEN, "test_images", name), "rb") as f:
            out.append((name, f.read()))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pillow_rgb():
    """name -> np.asarray(Image.open(f).convert("RGB")), computed once."""
    from PIL import Image

    return {name: np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8) for name, data in cases()}
