"""Inputs of the split Huffman decode tests (test_jpeg_split_cpu.py, test_jpeg_split_gpu.py): files WITHOUT restart
markers, so that the whole scan is one interval, each at most 60 KB.  Not a test module."""
import functools

import numpy as np

import jpeg_inputs as J

SIDES = ((33, 15), (97, 131), (131, 250), (256, 256))
CONTENTS = ("noise", "gradient", "checker", "flat", "stripes", "photo")
MAX_BYTES = 60 << 10


def content(kind, w, h, seed):
    if kind in J.CONTENTS:
        return J.content(kind, w, h, seed)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "flat":
        return np.full((h, w, 3), 37 + 11 * seed % 200, dtype=np.uint8)
    if kind == "stripes":  # 8-pixel stripes: every block row repeats, a guessed state never meets the true one
        return np.repeat((((x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, -1)
    # "photo": smooth structure plus mild noise
    base = 128 + 70 * np.sin(x / 17.0 + seed) * np.cos(y / 23.0) + 40 * np.sin((x + 2 * y) / 41.0)
    img = base[..., None] + np.asarray([0, 12, -9]) + rng.normal(0, 6, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, jpeg bytes)]: every side x content, restart interval 0; sampling, quality and table optimisation rotate so that every
    value of each occurs with every content and every side.  Files above 60 KB (noise at high quality on the large sides) are
    encoded again at the next lower quality."""
    out, i = [], 0
    for si, (w, h) in enumerate(SIDES):
        for ci, kind in enumerate(CONTENTS):
            for rep in range(2):
                s = J.SAMPLINGS[(i + si) % 4]
                qi = (si + ci + 2 * rep) % 4
                opt = bool((si + ci + rep) % 2)
                data = J.encode(content(kind, w, h, i), s, J.QUALITIES[qi], opt, 0)
                while len(data) > MAX_BYTES and qi > 0:
                    qi -= 1
                    data = J.encode(content(kind, w, h, i), s, J.QUALITIES[qi], opt, 0)
                out.append((f"{w}x{h}-s{s}-{kind}-q{J.QUALITIES[qi]}-o{int(opt)}-r0", data))
                i += 1
    out.append(two_subsequences())
    return tuple(out)


def entropy_bytes(data):
    """Entropy-coded bytes of a file without restart markers: what lies between the SOS header and the EOI."""
    at = data.index(b"\xff\xda")
    return len(data) - 2 - (at + 2 + int.from_bytes(data[at + 2:at + 4], "big"))


def two_subsequences():
    """A file whose one interval is EXACTLY 64 bytes long: two sub-sequences at split_bytes 32, the only length that gives two.  Found
    by a fixed search over quality and seed (16 x 16 gray noise lies around 64 bytes near quality 20)."""
    for q in range(12, 40):
        for seed in range(40):
            data = J.encode(J.content("noise", 16, 16, 1000 + seed), "L", q, False, 0)
            if entropy_bytes(data) == 64:
                return f"16x16-sL-noise-q{q}-o0-r0-e64", data
    raise AssertionError("no 64-byte scan among the candidates")


@functools.lru_cache(maxsize=None)
def pillow_rgb():
    import io

    from PIL import Image

    return {name: np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8) for name, data in cases()}
