"""The batched projection tail (tail_kernels.hip: tail_proj_batched_kernel) against the per-sample one (tail_proj_kernel).

launch_tail runs the batched kernel (8 samples per workgroup) from B * d * E >= 2^26 multiply-adds on and the per-sample kernel
below.  Both must write the same bytes: the embeddings of one batch are compared, bitwise, with the same samples encoded in
chunks of two (always the per-sample kernel; a chunk of ONE would take the split-K single-query GEMMs, which differ by summation
order, so an odd batch ends with an overlapping chunk).  Batch sizes per tower: the last one below the switch (per-sample on
both sides), the first one at it, and one above it that is not a multiple of 8 (a short last workgroup).  Which kernel the
encoder picks for a shape is asked from the library (clipx_tail_device with rows_per_workgroup = -1), not assumed, and the two
kernels are also run on the same rows directly (rows_per_workgroup = 0 / 8 / 16)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MIN_WORK = 1 << 26


def _switch(d, E):
    return -(-MIN_WORK // (d * E))


def _chunks_of_two(B):
    return [(o, o + 2) for o in range(0, B - 1, 2)] + ([(B - 2, B)] if B % 2 else [])


@pytest.fixture(scope="module")
def inputs():
    from oracle.clip_oracle import synth_pixels_u8, synth_tokens

    return {"image": synth_pixels_u8(256, size=224, seed=100), "text": synth_tokens(256, 77, 49408, seed=101)}


def _query(lib, B, d, E):
    import torch

    t = torch.zeros(8, device="cuda")
    p = C.c_void_p(t.data_ptr())  # (a query launches nothing; the pointers only have to be non-null)
    return lib.clipx_tail_device(0, p, p, p, p, p, None, p, B, d, E, C.c_float(1e-5), -1, None)


@pytest.mark.parametrize("d,E", [(512, 512), (768, 512), (768, 768), (1024, 768)])
@pytest.mark.parametrize("B", [2, 8, 9, 27, 256])
def test_tail_kernels_write_the_same_bytes(lib, B, d, E):
    """The per-sample kernel and the batched one (8 and 16 rows per workgroup) on the same pooled rows: fp16 and f32 outputs bitwise."""
    import torch

    g = torch.Generator(device="cpu").manual_seed(B * 7 + d + E)
    x = (torch.randn(B, d, generator=g) * 3).to(torch.float16).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).cuda(), (0.1 * torch.randn(d, generator=g)).cuda()
    proj = (torch.randn(E, d, generator=g) * d ** -0.5).to(torch.bfloat16).cuda()
    outs = []
    for rows in (0, 8, 16):
        o16 = torch.full((B, E), float("nan"), dtype=torch.float16, device="cuda")
        o32 = torch.full((B, E), float("nan"), dtype=torch.float32, device="cuda")
        scratch = torch.empty(B * E, dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.clipx_tail_device(0, C.c_void_p(x.data_ptr()), C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()),
                                   C.c_void_p(proj.data_ptr()), C.c_void_p(o16.data_ptr()), C.c_void_p(o32.data_ptr()),
                                   C.c_void_p(scratch.data_ptr()), B, d, E, C.c_float(1e-5), rows, C.c_void_p(st))
        assert rc == 0, lib.clipx_last_error()
        torch.cuda.synchronize()
        outs.append((o16.cpu().numpy().view(np.uint16), o32.cpu().numpy()))
    ref16, ref32 = outs[0]
    assert np.isfinite(ref32).all() and np.allclose(np.linalg.norm(ref32, axis=1), 1.0, atol=1e-5)
    for rows, (o16, o32) in zip((8, 16), outs[1:]):
        assert np.array_equal(o32.view(np.uint32), ref32.view(np.uint32)), f"{rows} rows per workgroup: f32 rows differ"
        assert np.array_equal(o16, ref16), f"{rows} rows per workgroup: fp16 rows differ"


def _check(enc, inputs, tower, B, lib, batched):
    fn = enc.encode_image if tower == "image" else enc.encode_text
    d = enc.arch.v_width if tower == "image" else enc.arch.t_width
    assert _query(lib, B, d, enc.arch.embed_dim) == (8 if batched else 0), "the batch sizes of this test were chosen around the switch"
    assert _query(lib, 2, d, enc.arch.embed_dim) == 0
    x = np.ascontiguousarray(inputs[tower][:B])
    assert B <= enc.max_batch
    whole16, whole32 = fn(x), fn(x, f32=True)
    assert np.isfinite(whole32).all()
    for lo, hi in _chunks_of_two(B):
        part = np.ascontiguousarray(x[lo:hi])
        assert np.array_equal(fn(part, f32=True).view(np.uint32), whole32[lo:hi].view(np.uint32)), f"{tower} B={B}: f32 rows {lo}..{hi - 1}"
        assert np.array_equal(fn(part).view(np.uint16), whole16[lo:hi].view(np.uint16)), f"{tower} B={B}: fp16 rows {lo}..{hi - 1}"


# ViT-B/32: E = 512, d = 768 (image: switch at B = 171) / 512 (text: switch at B = 256, the largest batch of one launch)
@pytest.mark.parametrize("tower,B", [("image", 170), ("image", 171), ("image", 173), ("text", 255), ("text", 256)])
def test_batched_tail_equals_per_sample_tail_vit_b32(lib, inputs, tower, B):
    from clip_retrieval_amd.encoder import get_encoder

    enc = get_encoder("random:ViT-B/32")
    sw = _switch(enc.arch.v_width if tower == "image" else enc.arch.t_width, enc.arch.embed_dim)
    _check(enc, inputs, tower, B, lib, batched=B >= sw)


@pytest.fixture(scope="module")
def l14_shaped():
    """The tail dimensions of ViT-L/14 (E = 768, d = 1024 / 768) on towers of two layers: the tail does not see the depth."""
    from dataclasses import replace

    from clip_retrieval_amd.encoder import ARCHS, ClipEncoder, random_blob

    arch = replace(ARCHS["ViT-L/14"], v_layers=2, t_layers=2)
    enc = ClipEncoder(arch, random_blob(arch, 1), 0)
    yield enc
    enc.close()


def test_batched_tail_equals_per_sample_tail_vit_l14_dimensions(lib, l14_shaped, inputs):
    """B = 115: above the switch of both towers (86 and 114), not a multiple of 8."""
    _check(l14_shaped, inputs, "image", 115, lib, batched=True)
    _check(l14_shaped, inputs, "text", 115, lib, batched=True)
