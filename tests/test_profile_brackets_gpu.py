"""The GEMM brackets of clipx_profile_enable: start / stop events on the kernels' own dispatches (the default) against marker
events recorded around every launch (OPT_PROF_MARKERS = 1, the form of the other kinds).  ViT-B/32, B = 16, one process.

A step = one image batch + one text batch.  GEMM launches per step, from the layer structure: the image tower has the patch
embedding + 12 blocks x (QKV, out-proj, fc1, fc2) = 49, the text tower 12 x 4 = 48.  Their flops are 2 M N K each; with the
last block pooled (the default) its out-proj / fc1 / fc2 run on the B pooled rows, and the ragged text tower (B > 8) runs on
sum(caption lengths) rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B, STEPS = 16, 3
KIND_GEMM, PROF_GEMM = 0, 2


@pytest.fixture(scope="module")
def enc():
    from clip_retrieval_amd.encoder import get_encoder

    e = get_encoder("random:ViT-B/32")
    yield e
    e.profile(0)
    e.profile_get(KIND_GEMM)
    e.set_option(e.OPT_PROF_MARKERS, 0)


@pytest.fixture(scope="module")
def batch(enc):
    from oracle.clip_oracle import synth_pixels_u8, synth_tokens

    return synth_pixels_u8(B, size=enc.arch.image_size, seed=31), synth_tokens(B, enc.arch.ctx_len, enc.arch.vocab, seed=32)


def _expected(arch, ids):
    def tower(M, Bp, w, mlp, layers):
        full = 2.0 * M * w * (3 * w + w + 2 * mlp)
        last = 2.0 * M * w * 3 * w + 2.0 * Bp * w * (w + 2 * mlp)
        return (layers - 1) * full + last

    Tv = (arch.image_size // arch.patch_size) ** 2 + 1
    Kp = -(-3 * arch.patch_size ** 2 // 64) * 64
    rows_t = int((ids.argmax(axis=1) + 1).sum())
    flops = 2.0 * B * Tv * arch.v_width * Kp + tower(B * Tv, B, arch.v_width, arch.v_mlp, arch.v_layers)
    flops += tower(rows_t, B, arch.t_width, arch.t_mlp, arch.t_layers)
    return 1 + 4 * arch.v_layers + 4 * arch.t_layers, flops


def _run(enc, batch, markers, steps=STEPS, prof=PROF_GEMM):
    """`steps` steps under one form -> (launches, ms, flops, outputs of the last step)."""
    pix, ids = batch
    enc.set_option(enc.OPT_PROF_MARKERS, 1 if markers else 0)
    enc.profile(prof)
    try:
        for _ in range(steps):
            out = enc.encode_image(pix), enc.encode_text(ids)
    finally:
        enc.profile(0)
    n, ms, fl = enc.profile_get(KIND_GEMM)
    return n, ms, fl, out


def test_counts_and_outputs_are_the_same_in_both_forms(enc, batch):
    launches, flops = _expected(enc.arch, batch[1])
    n0, _, f0, plain = _run(enc, batch, markers=False, prof=0)
    assert (n0, f0) == (0, 0.0)
    for markers in (False, True):
        n, ms, fl, out = _run(enc, batch, markers)
        assert n == STEPS * launches, (markers, n)
        assert fl == pytest.approx(STEPS * flops, rel=1e-12), (markers, fl)
        assert ms > 0.0
        for a, b in zip(out, plain):
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), f"markers={markers}: profiling changed the embeddings"


def test_dispatch_events_time_no_more_than_markers(enc, batch):
    """The marker form is the reference: five repeats, spread = max / min - 1.  A marker pair spans the scope's kernels AND the
    gaps around them; the dispatch form sums the kernels' own run times, so its total is positive and at most the markers' maximum
    widened by their own spread."""
    _run(enc, batch, markers=True)  # warm-up
    marker = [_run(enc, batch, markers=True)[1] for _ in range(5)]
    spread = max(marker) / min(marker) - 1.0
    disp = [_run(enc, batch, markers=False)[1] for _ in range(5)]
    print(f"GEMM ms per {STEPS} steps: markers {[round(v, 3) for v in marker]} (spread {spread:.3f}), "
          f"dispatch {[round(v, 3) for v in disp]}, ratio of the medians {np.median(disp) / np.median(marker):.3f}")
    assert min(disp) > 0.0
    assert max(disp) <= max(marker) * (1.0 + spread)


def test_event_pool_is_reused(enc, batch):
    """clipx_profile_get hands the events it has read back to the pool: further profiled steps create none."""
    for markers in (False, True):
        _run(enc, batch, markers, steps=1)
    created = enc.profile_events()
    assert created > 0
    for i in range(20):
        n, ms, _, _ = _run(enc, batch, markers=bool(i % 2), steps=1)
        assert n > 0 and ms > 0.0
    assert enc.profile_events() == created
