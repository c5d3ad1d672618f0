"""ViT-L/14@336px on the GPU: the long-sequence attention kernel (T = 289 .. 608, head dimension 64) against fp32 torch on the same
fp16 inputs, its online-softmax corners, the refusals, the old shapes' bits, and the 336-pixel encoder against the CPU oracle."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_short_bits.npz")
E_UNSUPPORTED = -5


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.fixture(scope="module")
def lib():
    import clip_retrieval_amd

    return clip_retrieval_amd.load_library()


def _inputs(B, T, H, dh=64):
    """test_attention's inputs (tests/test_clip_gpu.py): randn in fp16 from the CPU generator seeded T * 31 + H, q scaled by 2."""
    g = torch.Generator().manual_seed(T * 31 + H)
    qkv = (torch.randn(B * T, 3 * H * dh, generator=g)).to(torch.float16)
    qkv[:, : H * dh] *= 2.0
    return qkv


def _run(lib, qkv, B, T, H, causal=0):
    from clip_retrieval_amd._lib import check

    out = torch.empty(B * T, H * 64, dtype=torch.bfloat16, device="cuda")
    check(lib, lib.clipx_attention_device(0, _ptr(qkv), _ptr(out), B, T, H, causal, None), "clipx")
    torch.cuda.synchronize()
    return out


def _reference(qkv, B, T, H, dh=64, causal=0):
    """fp32 softmax(q k^T / sqrt(dh)) v on the same fp16 inputs -> ([B T, H dh] fp32, probabilities [B, H, T, T])"""
    q, k, v = qkv.float().view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    if causal:
        s = s + torch.full((T, T), float("-inf"), device=qkv.device).triu_(1)
    p = torch.softmax(s, -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh), p, s


def _assert_close(out, want, what):
    assert torch.isfinite(out.float()).all(), f"{what}: NaN or Inf in the output"
    err = (out.float() - want).abs()
    print(f"{what}: max abs err {err.max().item():.4g} mean {err.mean().item():.4g}")
    assert err.max() < 2e-2, f"{what}: max err {err.max().item():.4g} at {err.argmax().item()}"
    assert err.mean() < 2e-3, f"{what}: mean err {err.mean().item():.4g}"


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("B,T,H", [(2, 289, 2), (1, 320, 3), (2, 401, 2), (1, 577, 16), (2, 608, 2)])
def test_long_attention_vs_fp32(lib, B, T, H):
    """(2, 289, 2): the first length past the old limit, one real key in block 10; (1, 320, 3): whole blocks; (2, 401, 2): 13
    blocks, 17 real keys in the last; (1, 577, 16): the model's own; (2, 608, 2): the maximum, LDS full.  Reference and bars are
    test_attention's: fp32 torch on the same fp16 inputs, max abs error < 2e-2 and mean < 2e-3 on the bf16 output."""
    qkv = _inputs(B, T, H).cuda()
    out = _run(lib, qkv, B, T, H)
    want, _, _ = _reference(qkv, B, T, H)
    _assert_close(out, want, f"B={B} T={T} H={H}")


def test_long_attention_online_softmax_corners(lib):
    """Crafted logits at T = 577 (18 blocks of 32 keys + one key), one head, |v| <= 2.  Queries i % 3 == 0: key 576 -- the only
    real key of the last block -- has the largest logit by about 9 (more than 2 over every other key), after the sum has been built on smaller maxima;
    i % 3 == 1: key 0 has it, so the maximum never moves after the first block; i % 3 == 2: q = 8 k[j], a softmax that is one-hot
    to fp16 (every other P rounds to 0), j walking over all the blocks.  No NaN or Inf anywhere, test_attention's bars."""
    B, T, H, dh = 1, 577, 1, 64
    g = torch.Generator().manual_seed(577)
    u = torch.where(torch.rand(dh, generator=g) < 0.5, -1.0, 1.0)
    k = torch.randn(T, dh, generator=g)
    k *= 8.0 / k.norm(dim=1, keepdim=True)  # |k| = 8: a key's logit with 8 x itself is 64, with 8 x another key about N(0, 8)
    k[576], k[0] = 1.25 * u, -1.25 * u
    v = torch.randn(T, dh, generator=g).clamp_(-2, 2)
    q = torch.empty(T, dh)
    i = torch.arange(T)
    last, first, hot = i % 3 == 0, i % 3 == 1, i % 3 == 2
    noise = 0.25 * torch.randn(T, dh, generator=g)
    q[last] = 2.0 * (0.45 * u + noise[last])    # q scaled by 2 as test_attention does: logit 9 +- 1.6 against N(0, 1) elsewhere
    q[first] = 2.0 * (-0.45 * u + noise[first])
    target = (i * 7) % T
    target[575], target[2] = 576, 0             # and the two planted keys: the single key of the last block, the first key
    q[hot] = 8.0 * k[target[hot]]               # the "q scaled by 8" group
    qkv = torch.cat([q, k, v], 1).to(torch.float16).cuda()
    want, p, s = _reference(qkv, B, T, H)
    p, s = p[0, 0], s[0, 0]
    # the crafting holds in the reference itself
    others = s.clone()
    others[:, 576] = float("-inf")
    assert (s[last.cuda(), 576] - others[last.cuda()].max(-1).values).min() > 2.0
    others = s.clone()
    others[:, 0] = float("-inf")
    assert (s[first.cuda(), 0] - others[first.cuda()].max(-1).values).min() > 2.0
    ph = p[hot.cuda()]
    assert (ph.argmax(-1).cpu() == target[hot]).all() and ph.max(-1).values.min() > 1 - 1e-6
    second = ph.clone().scatter_(1, ph.argmax(-1, keepdim=True), 0.0).max()
    assert second < 2.0 ** -25, "every P outside the one key must round to 0 in fp16"
    assert set((target[hot] // 32).tolist()) == set(range(19)), "the one-hot key visits every key block"
    out = _run(lib, qkv, B, T, H)
    _assert_close(out, want, "crafted T=577")
    # a one-hot row is its key's v rounded to bf16: relative error 2^-9 of the rounding, and about 1e-5 of the row sum (the one
    # P is exp2 of the rounding residue of S c - m c, as in attention_kernel, so the sum is 1 only to fp32 rounding of m c)
    got_hot = out[hot.cuda()].float().cpu()
    v_hot = v.to(torch.float16).float()[target[hot]]
    assert ((got_hot - v_hot).abs() <= v_hot.abs() * 2.0 ** -8).all()


def test_refusals_launch_nothing(lib):
    """T = 609 at dh 64, T = 300 causal and T = 577 at dh 80 are CLIPX_E_UNSUPPORTED with a message that names the limit, the output
    buffer is untouched, and a T = 257 result read before and after is the same: the device is still healthy."""
    B, H = 2, 16
    qkv257 = _inputs(B, 257, H).cuda()
    before = _run(lib, qkv257, B, 257, H)
    big = torch.zeros(609, 3 * 80, dtype=torch.float16, device="cuda")
    out = torch.full((609, 80), 7.0, dtype=torch.bfloat16, device="cuda")
    assert lib.clipx_attention_device(0, _ptr(big), _ptr(out), 1, 609, 1, 0, None) == E_UNSUPPORTED
    assert "608" in lib.clipx_last_error().decode()
    assert lib.clipx_attention_dh_device(0, _ptr(big), _ptr(out), 1, 609, 1, 64, 0, None) == E_UNSUPPORTED
    assert lib.clipx_attention_device(0, _ptr(big), _ptr(out), 1, 300, 1, 1, None) == E_UNSUPPORTED
    assert "288" in lib.clipx_last_error().decode()
    assert lib.clipx_attention_dh_device(0, _ptr(big), _ptr(out), 1, 300, 1, 64, 1, None) == E_UNSUPPORTED
    assert lib.clipx_attention_dh_device(0, _ptr(big), _ptr(out), 1, 577, 1, 80, 0, None) == E_UNSUPPORTED
    assert "288" in lib.clipx_last_error().decode()
    torch.cuda.synchronize()
    assert (out.float() == 7.0).all()
    after = _run(lib, qkv257, B, 257, H)
    assert torch.equal(before.view(torch.int16), after.view(torch.int16))
    want, _, _ = _reference(qkv257, B, 257, H)
    _assert_close(after, want, "T=257 after the refusals")


def test_old_shapes_give_the_old_bits(lib):
    """Everything at T <= 288 runs the kernels it ran before: the outputs at (2, 257, 16, 64) and (3, 77, 12, 64, causal) on
    test_attention's inputs have the SHA-256 recorded in tests/golden/attention_short_bits.npz from the library of the commit
    before the long-sequence kernel.  Recipe: build that commit's csrc into a library of its own, then on the MI355X
        python tools/record_attention_short_bits.py --lib <that libclipx.so> --out tests/golden/attention_short_bits.npz
    (the tool holds the same input recipe; the file also keeps the digest of the inputs, asserted first here, so a change of
    the generator shows up as that and not as a change of the kernels)."""
    gold = np.load(GOLDEN)
    for name, (B, T, H, causal) in (("b2_t257_h16", (2, 257, 16, 0)), ("b3_t77_h12_causal", (3, 77, 12, 1))):
        qkv = _inputs(B, T, H)
        assert hashlib.sha256(qkv.numpy().tobytes()).digest() == gold["in_" + name].tobytes(), f"{name}: the inputs differ from the recorded ones"
        out = _run(lib, qkv.cuda(), B, T, H, causal)
        bits = out.view(torch.int16).cpu().numpy()
        assert np.array_equal(bits.reshape(-1)[:256], gold["head_" + name]), f"{name}: first 256 outputs differ"
        assert hashlib.sha256(bits.tobytes()).digest() == gold["out_" + name].tobytes(), f"{name}: output bits differ from the parent's"


# ------------------------------------------------------------------------------------------ the encoder
def _arch336():
    from oracle.clip_oracle import ClipArch

    return ClipArch(image_size=336, v_layers=2, t_layers=2)


def _product_arch(arch):
    from clip_retrieval_amd.encoder import ClipArch

    return ClipArch(**{k: getattr(arch, k) for k in ClipArch.__dataclass_fields__})


@pytest.fixture(scope="module")
def tiny336():
    """Two layers per tower at ViT-L/14 widths and 336 pixels (577 image tokens); oracle weights, seed 0."""
    from clip_retrieval_amd.encoder import ClipEncoder
    from oracle.clip_oracle import HFClipOracle

    arch = _arch336()
    oracle = HFClipOracle(arch, seed=0)
    blob = oracle.export_blob()
    enc = ClipEncoder(_product_arch(arch), blob, 0)
    yield arch, oracle, enc, blob
    enc.close()


@pytest.mark.parametrize("B", [1, 2, 9])
def test_encoder_336_parity_vs_oracle(tiny336, B):
    """B = 1 and 2 replay from graphs (M = 577 and 1 154 rows), B = 9 leaves the graph path (M = 5 193).  The bars are exactly those
    of test_encoder_parity_vs_oracle."""
    from oracle.clip_oracle import mapper_semantics, normalise_u8_nhwc, parity_gate, synth_pixels_u8, synth_tokens

    arch, oracle, enc, _ = tiny336
    u8 = synth_pixels_u8(B, size=336, seed=B)
    assert u8.shape == (B, 336, 336, 3)
    pix = normalise_u8_nhwc(u8)
    ids = synth_tokens(B, seed=10 + B)
    want_i16, want_i32 = mapper_semantics(oracle.encode_image(torch.from_numpy(pix)))
    _, want_t32 = mapper_semantics(oracle.encode_text(torch.from_numpy(ids)))
    got_i = enc.encode_image(pix)
    got_t = enc.encode_text(ids)
    assert got_i.dtype == np.float16 and got_i.shape == (B, arch.embed_dim) and got_i.flags["C_CONTIGUOUS"]
    parity_gate(got_i, want_i32, "336 image")
    parity_gate(got_t, want_t32, "336 text")
    assert np.allclose(np.linalg.norm(got_i.astype(np.float32), axis=1), 1, atol=2e-3)
    assert np.abs(got_i.astype(np.float32) - want_i16.astype(np.float32)).max() < 0.02
    got_u8 = enc.encode_image(u8)
    assert _cos(got_u8, got_i).min() > 1 - 1e-4


def test_pooled_last_block_336_equals_the_full_block(tiny336):
    """The last image block asks the attention for query block 0 only (q_blocks = 1: one wave of the long-sequence kernel works).
    Against an encoder with pool_last_block off (CLIPX_FULL_LAST_BLOCK=1, the full launch): batches of two and more give the same
    BYTES -- the rows of query block 0 are bit-equal between the two launches, and a GEMM row does not depend on the rows it
    travels with -- and the single query's split-K path the same embedding to cosine 1 - 1e-5 (the existing test's bar)."""
    from clip_retrieval_amd.encoder import ClipEncoder
    from oracle.clip_oracle import normalise_u8_nhwc, synth_pixels_u8

    arch, _, enc, blob = tiny336
    os.environ["CLIPX_FULL_LAST_BLOCK"] = "1"
    try:
        full = ClipEncoder(_product_arch(arch), blob, 0)
    finally:
        os.environ.pop("CLIPX_FULL_LAST_BLOCK")
    try:
        assert enc.get_option(enc.OPT_POOL_LAST_BLOCK) == 1 and full.get_option(full.OPT_POOL_LAST_BLOCK) == 0
        for B in (2, 9):
            pix = normalise_u8_nhwc(synth_pixels_u8(B, size=336, seed=40 + B))
            assert np.array_equal(enc.encode_image(pix), full.encode_image(pix)), f"336 image B={B}"
        pix = normalise_u8_nhwc(synth_pixels_u8(1, size=336, seed=3))
        assert _cos(enc.encode_image(pix), full.encode_image(pix).astype(np.float32)).min() > 1 - 1e-5
    finally:
        full.close()


def test_clip_mapper_takes_the_336_model(tiny336):
    """ClipMapper on the 336-pixel model, the encoder registered under the model's name as the drop-in test registers its own: a
    batch of 3 images of 336 x 336 returns float16 [3, 768]."""
    from clip_retrieval_amd.encoder import ARCHS, register_encoder, resolve_arch_name
    from clip_retrieval_amd.mapper import ClipMapper
    from oracle.clip_oracle import mapper_semantics, normalise_u8_nhwc, parity_gate, synth_pixels_u8, synth_tokens

    arch, oracle, enc, _ = tiny336
    name = resolve_arch_name("open_clip:ViT-L-14-336/openai")
    assert name == "ViT-L/14@336px" and ARCHS[name].image_size == enc.arch.image_size and ARCHS[name].v_tokens == enc.arch.v_tokens
    register_encoder(name, enc)
    mapper = ClipMapper(enable_image=True, enable_text=True, enable_metadata=False, use_mclip=False,
                        clip_model="registered:" + name, use_jit=True, mclip_model="", warmup_batch_size=1)
    pix = torch.from_numpy(normalise_u8_nhwc(synth_pixels_u8(3, size=336, seed=23)))
    ids = torch.from_numpy(synth_tokens(3, seed=33)).long()
    out = mapper({"image_tensor": pix, "text_tokens": ids, "image_filename": ["0.jpg", "1.jpg", "2.jpg"], "text": ["a", "b", "c"]})
    assert out["image_embs"].shape == (3, 768) and out["image_embs"].dtype == np.float16
    assert out["text_embs"].shape == (3, 768) and out["text_embs"].dtype == np.float16
    parity_gate(out["image_embs"], mapper_semantics(oracle.encode_image(pix))[1], "336 mapper image")
